"""csr5hip_attention_backward (``A.attentionBackward``) and ``autograd.fused_attention(..., backward="fused")`` on the GPU: dQ, dK
and dV against the float64 torch reference of tests/test_gpu_attention_autograd.py, gradcheck, the same bits on every layout,
leading dimension and alignment, poisoned outputs and guard bytes, every subset of the outputs, an untouched handle, special
values, graph capture, and agreement with the ``"recompute"`` route.

Line classes of the two kernels and where they are met.  The row kernel (dQ, the workspace): rows of at most 16 entries (kat0,
half-empty, ...), 17 .. 512 (aligned64, row 5 of the duplicates matrix), 513 .. 2 048 (aligned1024) and beyond (hub, two-hubs,
one-row).  The column kernel (dK, dV) decides by the COLUMN's length, and the zoo's columns are short: only the transposes of
aligned64 (columns of 64 entries), aligned1024 (1 024), two-hubs (5 000 and 7 000) and hub (9 000) reach its wavefront and
workgroup classes.  Widths 70 and 40 have a second column block; 300 has a second group of four blocks in every output.  None of these
lines sits ON a class edge and every line beyond 512 entries lies in workgroup 0: the edges, hubs in later workgroups, second
column blocks of width 1 and dQ, dK and dV bit for bit are in tests/test_gpu_attention_edges.py.

THE BOUND of the accuracy test.  tests/test_gpu_attention_autograd.py derives, for the unfused chain, |grad - ref| <= STAGES rho A
with A the gradient expression on absolute values and rho the largest relative error of a factor.  The fused backward is, per
entry e = (i, j) (csr5hip.h):  p_e = exp(s_e - M_i) / Z_i,  dp_e = dO[i, :] . V[j, :],  D_i = sum_row p dp,
ds_e = p_e (dp_e - D_i),  dQ = sum_row ds K,  dK = sum_column ds Q,  dV = sum_column p dO.  The factors and sums that carry a
rounding error, each relative to its own absolute-value expression:

    1  the outer p_e          rho (that module's: the scores' 2 sigma, the softmax's beta, gamma(L))
    2  dp_e                   gamma(d): a chain of d fused multiply-adds
    3  the p inside D_i       rho
    4  the product p dp       u
    5  the sum D_i            gamma(L) (the tree is no longer than the chain)
    6  the difference         u
    7  the product with p_e   u
    8  the final sum          gamma(L) for dQ, gamma(longest column) for dK and dV

so STAGES_B = 8 factors, each within rho_b = rho + gamma(d) + gamma(longest column) (Q, K, V and dO are exact inputs; dV has
only stages 1 and 8).  To first order |grad - ref| <= STAGES_B rho_b A; the terms dropped are at most
(STAGES_B rho_b)**2 / (2 (1 - STAGES_B rho_b)) of A, under 1/126 of the allowance while STAGES_B rho_b <= 2**-6, which the test
asserts before it compares: a condition on the data, evaluated in numpy for every case of this file beforehand.  Q carries the
usual scaling of attention, 1 / sqrt(k) (entries in [-2, 2) / sqrt(k)): with entries of Q in [-2, 2) at k = 300 the scores'
own error, gamma(300) sum |Q K|, alone gives STAGES_B rho_b = 5e-2 in fp32.  With it the largest value of the file is hub in
fp32 at (k, d) = (70, 40) (gamma(9 000) enters three times), which stays below the cap, so no case is moved to (8, 16).  The two
added gammas get that module's factors too ((1 + 2**-10), and 2 in fp64 where the reference obeys the same bound)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_attention_autograd import STAGES, _allowances, _index, _reference, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, Path, _bits, _close  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
STAGES_B = 8
FIRST_ORDER = 2.0 ** -6
NAMES = ("kat0", "tiny-p1", "half-empty", "hub", "aligned64", "aligned1024", "two-hubs", "one-row", "single-nnz")
TRANSPOSED = ("hub", "two-hubs", "aligned1024", "aligned64")
KD = ((1, 1), (3, 5), (8, 16), (70, 40))
KD_WIDE = ((5, 300), (300, 5))
POISON = -777.25
BY_NAME = {p.name: p for p in PATHS}
SIGMA_PATHS = [Path(f"sigma{s}", s, H.SPMV_FUSED) for s in (4, 7, 16, 32)]


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def transpose(mat):
    """A^T in CSR, every column's entries in A's CSR order: a stable sort of the entries by column"""
    rows = np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))
    cols = mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T")


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["duplicates"] = S.duplicates_matrix()
    for name in TRANSPOSED:
        z[name + "^T"] = transpose(z[name])
    return z


def _matrices():
    return [_zoo()[n] for n in NAMES + ("duplicates",) + tuple(n + "^T" for n in TRANSPOSED)]


def operands(mat, k, d, dtype, seed):
    """(Q, K, V, dO) in numpy: Q in [-2, 2) / sqrt(k), the others in [-1, 1)"""
    rng = np.random.default_rng([seed, k, d, 64 if dtype == np.float64 else 32])
    u = lambda shape: rng.uniform(-1, 1, size=shape).astype(dtype)  # noqa: E731
    return u((mat.m, k)) * dtype(2 / np.sqrt(max(k, 1))), u((mat.n, k)), u((mat.n, d)), u((mat.m, d))


def _operands(mat, k, d, dtype, seed):
    return tuple(torch.from_numpy(t).to(DEV) for t in operands(mat, k, d, dtype, seed))


def _open(mat, dtype, path=None, companion=True):
    """a converted handle with the path's options (what spmv() then selects is not this file's business), with its companion"""
    path = path or Path("backward", AUTO, H.SPMV_FUSED)
    rp = torch.from_numpy(mat.row_ptr.astype(np.int32)).to(DEV)
    ci = torch.from_numpy(mat.col.astype(np.int32)).to(DEV)
    va = torch.ones(mat.nnz, dtype=_tdt(dtype), device=DEV)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    A._arrays = (rp, ci, va)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    assert A.setSigma(path.sigma) == 0
    assert A.setSpmvMode(path.mode) == 0
    for setter, value in path.opts:
        assert getattr(A, setter)(value) == 0, (setter, _capi.last_error())
    assert A.asCSR5() == 0, _capi.last_error()
    if companion:
        assert A.buildTranspose() == 0, _capi.last_error()
    return A


def _backward(A, mat, Q, K, V, dO, want=(True, True, True)):
    """A.attentionBackward into NaN-poisoned outputs and a NaN-poisoned workspace: every wanted element must be written"""
    nan = float("nan")
    shapes = ((mat.m, Q.shape[1]), (mat.n, Q.shape[1]), (mat.n, V.shape[1]))
    outs = [torch.full(s, nan, dtype=Q.dtype, device=DEV) if w else None for s, w in zip(shapes, want)]
    work = torch.full((4 * mat.m,), nan, dtype=Q.dtype, device=DEV) if want[1] or want[2] else None
    assert A.attentionBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return outs


def _empty(mat):
    rows = torch.from_numpy(np.diff(mat.row_ptr) == 0).to(DEV)
    cols = torch.from_numpy(np.bincount(mat.col[:mat.nnz], minlength=mat.n) == 0).to(DEV)
    return rows, cols, cols


def _bound(mat, Q, K, V, dO, dtype):
    """(references (dQ, dK, dV), allowances (dQ, dK, dV), STAGES_B rho_b): the module docstring's bound"""
    rows, cols = _index(mat)
    ref = _reference(mat, rows, cols, Q, K, V, dO)[1:]
    rho, _, a_Q, a_K, a_V = _allowances(mat, rows, cols, Q, K, V, dO, dtype)
    u = unit_roundoff(dtype)
    gamma = lambda n: n * u / (1 - n * u)  # noqa: E731
    longest = int(np.bincount(mat.col[:mat.nnz], minlength=1).max()) if mat.nnz else 0
    rho_b = rho + (gamma(V.shape[1]) + gamma(longest)) * (1 + 2.0 ** -10) * (2 if dtype == np.float64 else 1)
    scale = STAGES_B * rho_b / (STAGES * rho)
    return ref, tuple(a * scale for a in (a_Q, a_K, a_V)), STAGES_B * rho_b


def _check(mat, got, Q, K, V, dO, dtype, what):
    ref, allowed, first_order = _bound(mat, Q, K, V, dO, dtype)
    print(f"{what}: STAGES_B rho_b = {first_order:.3e}")
    assert first_order <= FIRST_ORDER, (what, first_order)
    for g, r, a, e, name in zip(got, ref, allowed, _empty(mat), ("dQ", "dK", "dV")):
        if g is None:
            continue
        _within(g, r, a, f"{what} {name}")
        assert not _bits(g[e].cpu().numpy()).any(), (what, name)  # rows / columns without entries: exactly +0


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("kd", KD, ids=lambda kd: f"k{kd[0]}-d{kd[1]}")
def test_gradients_match_the_float64_reference(kd, dtype):
    for mi, mat in enumerate(_matrices()):
        k, d = kd
        Q, K, V, dO = _operands(mat, k, d, dtype, seed=100 + mi)
        A = _open(mat, dtype)
        got = _backward(A, mat, Q, K, V, dO)
        _close(A)
        _check(mat, got, Q, K, V, dO, dtype, f"{mat.name} {_dt(dtype)} k={k} d={d}")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("kd", KD_WIDE, ids=lambda kd: f"k{kd[0]}-d{kd[1]}")
def test_more_than_four_column_blocks(kd, dtype):
    """a width of 300: lines beyond 512 entries sweep the columns in groups of 256 (and recompute beyond 2 048 entries)"""
    k, d = kd
    for mi, name in enumerate(("aligned1024", "one-row", "aligned1024^T", "one-row^T")):
        mat = _zoo()[name] if name in _zoo() else transpose(_zoo()[name[:-2]])
        Q, K, V, dO = _operands(mat, k, d, dtype, seed=300 + mi)
        A = _open(mat, dtype)
        got = _backward(A, mat, Q, K, V, dO)
        _close(A)
        _check(mat, got, Q, K, V, dO, dtype, f"{mat.name} {_dt(dtype)} k={k} d={d}")


# ---- 2. gradcheck --------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_the_fused_backward():
    """fp64, torch's default tolerances, on the matrix with repeated pairs and empty rows at sigma = 4 (p >= 2); clones as in
    tests/test_gpu_attention_autograd.py (gradcheck perturbs through ``.data``)"""
    mat = S.duplicates_matrix()
    A = _open(mat, np.float64, Path("sigma4", 4, H.SPMV_FUSED), companion=False)
    assert A.info().p >= 2 and (np.diff(mat.row_ptr) == 0).any()
    rng = np.random.default_rng(3)
    Q, K, V = (torch.from_numpy(rng.uniform(-1, 1, size=s)).to(DEV).requires_grad_(True) for s in ((mat.m, 3), (mat.n, 3), (mat.n, 2)))
    assert torch.autograd.gradcheck(lambda q, k, v: autograd.fused_attention(A, q.clone(), k.clone(), v.clone(), backward="fused"),
                                    (Q, K, V))
    _close(A)


# ---- 3. the same bits on every layout ------------------------------------------------------------------------------------------
LAYOUT_NAMES = ("half-empty", "hub", "aligned1024^T")


@functools.lru_cache(maxsize=None)
def _default_bits(name, dtype):
    mat = _zoo()[name]
    Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=7)
    A = _open(mat, dtype, BY_NAME["fused-default"])
    got = _backward(A, mat, Q, K, V, dO)
    _close(A)
    return tuple(_bits(g.cpu().numpy()) for g in got)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATHS + SIGMA_PATHS, ids=lambda p: p.name)
def test_same_bits_on_every_path_and_sigma(path, dtype):
    for name in LAYOUT_NAMES:
        mat = _zoo()[name]
        Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=7)
        A = _open(mat, dtype, path)
        got = _backward(A, mat, Q, K, V, dO)
        _close(A)
        for g, want, what in zip(got, _default_bits(name, dtype), ("dQ", "dK", "dV")):
            assert np.array_equal(_bits(g.cpu().numpy()), want), (path.name, name, what)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_same_bits_for_column_slices_and_offset_pointers(dtype):
    """(k, d) = (8, 16): the contiguous operands take 16-byte loads; slices of wider tensors with odd leading dimensions and
    pointers one element into an allocation take element loads -- the same chains, the same bits"""
    for name in LAYOUT_NAMES:
        mat = _zoo()[name]
        ops = _operands(mat, 8, 16, dtype, seed=7)
        A = _open(mat, dtype, BY_NAME["fused-default"])

        def sliced(t, pad_left, pad_right):
            wide = torch.full((t.shape[0], pad_left + t.shape[1] + pad_right), POISON, dtype=t.dtype, device=DEV)
            wide[:, pad_left:pad_left + t.shape[1]] = t
            return wide, wide[:, pad_left:pad_left + t.shape[1]]

        def offset(t):
            flat = torch.full((t.numel() + 1,), POISON, dtype=t.dtype, device=DEV)
            flat[1:] = t.reshape(-1)
            return flat[1:].view(t.shape)
        blank = [torch.zeros(s, dtype=_tdt(dtype), device=DEV) for s in ((mat.m, 8), (mat.n, 8), (mat.n, 16))]
        ins = [sliced(t, l, r)[1] for t, (l, r) in zip(ops, ((3, 2), (1, 0), (0, 7), (2, 1)))]
        outs = [sliced(t, l, r) for t, (l, r) in zip(blank, ((2, 3), (0, 1), (5, 0)))]
        work = torch.empty(4 * mat.m + 1, dtype=_tdt(dtype), device=DEV)
        assert A.attentionBackward(*ins, *(o[1] for o in outs), work[1:]) == 0, _capi.last_error()
        outs_o = [offset(t) for t in blank]
        assert A.attentionBackward(*(offset(t) for t in ops), *outs_o, work[:-1]) == 0, _capi.last_error()
        torch.cuda.synchronize()
        _close(A)
        for (wide, view), off, want, (l, r), what in zip(outs, outs_o, _default_bits(name, dtype), ((2, 3), (0, 1), (5, 0)),
                                                          ("dQ", "dK", "dV")):
            assert np.array_equal(_bits(view.cpu().numpy()), want), (name, what, "slices")
            assert np.array_equal(_bits(off.cpu().numpy()), want), (name, what, "offset pointers")
            assert bool((wide[:, :l] == POISON).all()) and bool((wide[:, wide.shape[1] - r:] == POISON).all()), (name, what)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_row_alone_gives_the_dq_bits_it_has_inside_a_matrix(dtype):
    mat = _zoo()["two-hubs"]
    Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=9)
    A = _open(mat, dtype, companion=False)
    dQ = _backward(A, mat, Q, K, V, dO, want=(True, False, False))[0].cpu().numpy()
    _close(A)
    for r in (0, 3, 8):  # 5 000, 7 000 and 2 entries
        a, b = int(mat.row_ptr[r]), int(mat.row_ptr[r + 1])
        one = M.CsrMatrix(1, mat.n, np.array([0, b - a], dtype=np.int32), mat.col[a:b].copy(), np.ones(b - a), f"row{r}")
        A1 = _open(one, dtype, Path("sigma7", 7, H.SPMV_FUSED), companion=False)
        dQ1 = _backward(A1, one, Q[r:r + 1].clone(), K, V, dO[r:r + 1].clone(), want=(True, False, False))[0].cpu().numpy()
        _close(A1)
        assert np.array_equal(_bits(dQ1[0]), _bits(dQ[r])), r


# ---- 4. poison and guard -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_nothing_but_the_wanted_columns_is_written(dtype):
    for name in ("half-empty", "hub", "aligned64^T"):
        mat = _zoo()[name]
        k, d, pad, guard = 3, 5, 3, 64
        Q, K, V, dO = _operands(mat, k, d, dtype, seed=11)
        keep = [t.clone() for t in (Q, K, V, dO)]
        bufs, views = [], []
        for rows, width in ((mat.m, k), (mat.n, k), (mat.n, d)):
            buf = torch.full((guard + rows * (width + pad) + guard,), POISON, dtype=_tdt(dtype), device=DEV)
            bufs.append(buf)
            views.append(buf[guard:guard + rows * (width + pad)].view(rows, width + pad)[:, :width])
        work = torch.empty(4 * mat.m, dtype=_tdt(dtype), device=DEV)
        A = _open(mat, dtype)
        assert A.attentionBackward(Q, K, V, dO, views[0], views[1], views[2], work) == 0, _capi.last_error()
        torch.cuda.synchronize()
        _close(A)
        for buf, view, what in zip(bufs, views, ("dQ", "dK", "dV")):
            rows, width = view.shape
            whole = buf.cpu().numpy()
            body = whole[guard:-guard].reshape(rows, width + pad)
            assert (whole[:guard] == POISON).all() and (whole[-guard:] == POISON).all() and (body[:, width:] == POISON).all(), (name, what)
            assert not (body[:, :width] == POISON).any(), (name, what)  # every wanted element is written
        _check(mat, views, Q, K, V, dO, dtype, f"{name} {_dt(dtype)} strided outputs")  # (and empty rows / columns are +0)
        for t, t0 in zip((Q, K, V, dO), keep):
            assert torch.equal(t, t0)


# ---- 5. subsets of the outputs -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_every_subset_of_the_outputs_gives_the_bits_of_the_full_call(dtype):
    for name in ("half-empty", "two-hubs^T"):
        mat = _zoo()[name]
        Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=12)
        A = _open(mat, dtype)
        full = [_bits(g.cpu().numpy()) for g in _backward(A, mat, Q, K, V, dO)]
        for mask in range(1, 7):
            want = (bool(mask & 1), bool(mask & 2), bool(mask & 4))
            got = _backward(A, mat, Q, K, V, dO, want)
            for g, f, w in zip(got, full, want):
                assert (g is not None) == w
                if w:
                    assert np.array_equal(_bits(g.cpu().numpy()), f), (name, mask)
        assert A.attention_backward_ptr(Q, 8, K, 8, 8, V, 16, 16, dO, 16, None, 8, None, 8, None, 16, None) == 0  # nothing wanted
        _close(A)
        # dQ alone: no companion, no workspace, and none is built
        A = _open(mat, dtype, companion=False)
        assert A.info().transpose_built == 0
        dQ = _backward(A, mat, Q, K, V, dO, want=(True, False, False))[0]
        assert A.info().transpose_built == 0 and np.array_equal(_bits(dQ.cpu().numpy()), full[0])
        work = torch.empty(4 * mat.m, dtype=_tdt(dtype), device=DEV)
        assert A.attentionBackward(Q, K, V, dO, dK=torch.empty_like(K), work=work) == _capi.INVALID_ARGUMENT
        assert "csr5hip_build_transpose" in _capi.last_error() and A.info().transpose_built == 0  # never built lazily
        _close(A)


# ---- 6. the handle is untouched ------------------------------------------------------------------------------------------------
def _info_without_transpose(A):
    info = A.info()
    for f in ("transpose_built", "t_transpose_build_ms", "t_sigma", "t_p", "t_tail_partition_start", "t_column_slabs", "t_slab_hot",
              "t_x_window_active"):
        setattr(info, f, 0)
    return bytes(info)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_handle_is_untouched(dtype):
    mat = _zoo()["half-empty"]
    rng = np.random.default_rng(13)
    A = _open(mat, dtype, BY_NAME["fused-default"], companion=False)
    assert A.updateValues(torch.from_numpy(rng.uniform(-1, 1, size=mat.nnz).astype(dtype)).to(DEV)) == 0
    x = torch.from_numpy(rng.uniform(-1, 1, size=mat.n).astype(dtype)).to(DEV)

    def spmv():
        y = torch.full((mat.m,), 3.0, dtype=_tdt(dtype), device=DEV)
        assert A.setX(x) == 0 and A.spmv(1.0, y) == 0
        torch.cuda.synchronize()
        return _bits(y.cpu().numpy())
    y0, info0 = spmv(), _info_without_transpose(A)
    Q, K, V, dO = _operands(mat, 8, 16, dtype, seed=14)
    _backward(A, mat, Q, K, V, dO, want=(True, False, False))
    assert _info_without_transpose(A) == info0 and A.info().transpose_built == 0
    assert A.buildTranspose() == 0
    info1 = bytes(A.info())
    _backward(A, mat, Q, K, V, dO)
    assert bytes(A.info()) == info1
    assert np.array_equal(spmv(), y0)
    # the autograd route: the record of the handle's values stays empty, the values stay
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    autograd.fused_attention(A, q, k, v, backward="fused").backward(dO)
    torch.cuda.synchronize()
    assert getattr(A, "_autograd_key", None) is None and q.grad is not None and k.grad is not None and v.grad is not None
    assert np.array_equal(spmv(), y0) and bytes(A.info()) == info1
    _close(A)


# ---- 7. special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_k_zero_gives_column_sums_of_do_over_the_row_length(dtype):
    u = unit_roundoff(dtype)
    for name in ("half-empty", "hub", "aligned64^T"):
        mat = _zoo()[name]
        rows, cols = _index(mat)
        _, _, V, dO = _operands(mat, 1, 7, dtype, seed=15)
        none = lambda r: torch.zeros((r, 0), dtype=_tdt(dtype), device=DEV)  # noqa: E731
        A = _open(mat, dtype)
        dQ, dK, dV = _backward(A, mat, none(mat.m), none(mat.n), V, dO)
        _close(A)
        assert dQ.shape == (mat.m, 0) and dK.shape == (mat.n, 0)
        L = torch.from_numpy(np.diff(mat.row_ptr).astype(np.float64)).to(DEV)
        terms = dO.double()[rows] / L[rows][:, None]
        want = torch.zeros((mat.n, 7), dtype=torch.float64, device=DEV).index_add(0, cols, terms)
        wabs = torch.zeros((mat.n, 7), dtype=torch.float64, device=DEV).index_add(0, cols, terms.abs())
        # w = 1 and Z = L exactly; one reciprocal, one product, then a chain or tree of at most Lc terms: gamma(Lc + 2)
        n = float(np.bincount(mat.col[:mat.nnz], minlength=mat.n).max()) + 2
        _within(dV, want, (n * u / (1 - n * u)) * wabs * (2 if dtype == np.float64 else 1 + 2.0 ** -10), f"{name} k = 0")
        assert not _bits(dV[_empty(mat)[2]].cpu().numpy()).any()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_matrix_without_entries_gives_zeros(dtype):
    mat = zoo.empty_matrix()
    A = _open(mat, dtype)
    Q, K, V, dO = _operands(mat, 4, 6, dtype, seed=16)
    for g, shape in zip(_backward(A, mat, Q, K, V, dO), ((mat.m, 4), (mat.n, 4), (mat.n, 6))):
        assert g.shape == shape and not _bits(g.cpu().numpy()).any()
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_non_finite_rows_stay_in_their_rows_and_their_columns(dtype):
    """Row b has a NaN in Q: NaN in its dQ row and in the dK and dV rows of exactly the columns it stores.  Q[a, 0] = -huge
    against K[:, 0] in {0, 32}: the entries of row a whose column has 32 overflow to -Inf and have p = +0, so everything else
    equals the gradients on the matrix without those entries and without row b, within that matrix' bound.  The reference
    keeps Q[a, 0] = -huge: it multiplies K[:, 0] = 0 in every entry of row a that is left, so it moves no score, but it is
    the factor of ds in column 0 of dK (no overflow: |ds| <= p (|dp| + |D|) <= 12 p with d = 6, a row's p sum to 1, and 12 huge
    is finite).  Only the NaN of row b, which has no entry left, is replaced."""
    mat = S.duplicates_matrix()
    lens = np.diff(mat.row_ptr)
    rows_np = S.rows_of(mat)
    huge = -1e307 if dtype == np.float64 else -2e37  # (32 huge overflows, 12 huge does not)
    a = int(np.flatnonzero(lens >= 6)[0])
    b = next(int(r) for r in np.flatnonzero(lens >= 2) if r != a)
    cols_a, cols_b = (mat.col[mat.row_ptr[r]:mat.row_ptr[r + 1]] for r in (a, b))
    masked_cols = sorted(set(cols_a.tolist()))[:2]
    Q, K, V, dO = _operands(mat, 4, 6, dtype, seed=17)
    K[:, 0] = 0
    K[torch.tensor(masked_cols, device=DEV), 0] = 32
    Q[a, 0] = huge
    benign = Q.clone()  # (before the NaN)
    Q[b, 1] = float("nan")
    A = _open(mat, dtype)
    dQ, dK, dV = _backward(A, mat, Q, K, V, dO)
    _close(A)
    in_b = torch.zeros(mat.n, dtype=torch.bool, device=DEV)
    in_b[torch.from_numpy(cols_b.astype(np.int64)).to(DEV)] = True
    not_b = torch.ones(mat.m, dtype=torch.bool, device=DEV)
    not_b[b] = False
    assert bool(torch.isnan(dQ[b]).all()) and bool(torch.isnan(dK[in_b]).all()) and bool(torch.isnan(dV[in_b]).all())
    assert bool(torch.isfinite(dQ[not_b]).all()) and bool(torch.isfinite(dK[~in_b]).all()) and bool(torch.isfinite(dV[~in_b]).all())
    keep = (rows_np != b) & ~((rows_np == a) & np.isin(mat.col[:mat.nnz], masked_cols))
    assert 0 < int(((rows_np == a) & keep).sum()) < cols_a.size
    rp = np.zeros(mat.m + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(rows_np[keep], minlength=mat.m))
    rest = M.CsrMatrix(mat.m, mat.n, rp, mat.col[:mat.nnz][keep].copy(), np.ones(int(keep.sum())), "rest")
    ref, allowed, first_order = _bound(rest, benign, K, V, dO, dtype)
    assert first_order <= FIRST_ORDER
    _within(dQ[not_b], ref[0][not_b], allowed[0][not_b], "dQ beside the NaN row")
    _within(dK[~in_b], ref[1][~in_b], allowed[1][~in_b], "dK beside the NaN row's columns")
    _within(dV[~in_b], ref[2][~in_b], allowed[2][~in_b], "dV beside the NaN row's columns")


# ---- 8. graph capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_first_backward_is_captured_in_a_graph(dtype):
    """two kernels on the handle's stream; the very first backward of the handle is the captured one (enqueue-only from the
    first call: a host synchronisation or an allocation inside the call would break the capture)"""
    mat = _zoo()["half-empty"]
    A = _open(mat, dtype, BY_NAME["fused-default"])
    Q, K, V, dO = _operands(mat, 13, 20, dtype, seed=18)
    outs = [torch.full(s, POISON, dtype=_tdt(dtype), device=DEV) for s in ((mat.m, 13), (mat.n, 13), (mat.n, 20))]
    work = torch.empty(4 * mat.m, dtype=_tdt(dtype), device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.attentionBackward(Q, K, V, dO, *outs, work) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    replayed = []
    news = [_operands(mat, 13, 20, dtype, seed=19 + i)[3] for i in range(2)]
    for dOn in news:
        dO.copy_(dOn)  # changed in place: the graph reads the same address
        for o in outs:
            o.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed.append([_bits(o.cpu().numpy()).copy() for o in outs])
    del graph
    assert A.setStream(None) == 0
    for dOn, got in zip(news, replayed):
        for e, g in zip(_backward(A, mat, Q, K, V, dOn), got):
            assert np.array_equal(_bits(e.cpu().numpy()), g)
    assert not np.array_equal(replayed[0][0], replayed[1][0])
    _close(A)


# ---- 9. the recompute route ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_fused_backward_agrees_with_the_recompute_route(dtype):
    """both routes obey their bound against the same float64 reference, so they differ by at most the sum of the two"""
    rng = np.random.default_rng(21)
    for mat in (_zoo()["half-empty"], _zoo()["hub"], _zoo()["duplicates"]):
        rows, cols = _index(mat)
        Q, K, V, dO = _operands(mat, 8, 5, dtype, seed=int(rng.integers(1 << 30)))
        got = {}
        for mode in ("fused", "recompute"):
            A = _open(mat, dtype, companion=False)
            q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
            out = autograd.fused_attention(A, q, k, v, backward=mode)
            out.backward(dO)
            torch.cuda.synchronize()
            assert A.info().transpose_built == 1  # K and V need gradients: built by the wrapper, once
            got[mode] = (q.grad, k.grad, v.grad)
            _close(A)
        _, allowed_b, first_order = _bound(mat, Q, K, V, dO, dtype)
        assert first_order <= FIRST_ORDER
        allowed_r = _allowances(mat, rows, cols, Q, K, V, dO, dtype)[2:]
        for f, r, ab, ar, what in zip(got["fused"], got["recompute"], allowed_b, allowed_r, ("dQ", "dK", "dV")):
            _within(f, r.double(), ab + ar, f"{mat.name} {_dt(dtype)} fused against recompute {what}")
