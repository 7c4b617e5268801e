"""csr5hip_mha / csr5hip_mha_backward (``A.mha``, ``A.mhaBackward``) and ``autograd.multihead_attention`` on the GPU.  The calls
are DEFINED by reference: head h of the packed call has, bit for bit, what the single-head call writes on that head's column
slices.  So most tests compare bits with ``A.attention`` / ``A.attentionBackward`` on slices of the same packed tensors; one
test goes to the float64 torch reference with the bound of tests/test_gpu_attention_autograd.py, so that this file does not rest
on the single-head kernel alone.

Shapes (heads, k, d) and why: (1, 8, 16) the single-head instantiation; (2, 8, 16) every slice 16-byte aligned: 16-byte loads;
(3, 3, 5) element loads; (3, 10, 6) in fp32 and (3, 5, 6) in fp64: head 0 is 16-byte aligned and head 1 is not; (5, 1, 1);
(2, 13, 70) a second column block per head.  With three heads the head groups hold two heads and one; no (lines, heads) of this
file gives a group more than two heads.  Groups of three heads and of all heads, the staged columns reused by the later heads at
exactly 512 and 2 048 entries, hubs in later workgroups and ``mhaBackward`` against the float64 reference are in
tests/test_gpu_attention_edges.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import _allowances, _index, _open, _reference, _uniform, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, Path, _bits, _close, _handle  # noqa: E402

RHO_MAX = 2.0 ** -6
POISON = -777.25
BY_NAME = {p.name: p for p in PATHS}
NAMES = ("half-empty", "aligned64", "aligned1024", "two-hubs", "duplicates")


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _shapes(dtype):
    trap = (3, 10, 6) if dtype == np.float32 else (3, 5, 6)
    return ((1, 8, 16), (2, 8, 16), (3, 3, 5), trap, (5, 1, 1), (2, 13, 70))


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["duplicates"] = S.duplicates_matrix()
    return z


def _operands(mat, heads, k, d, dtype, seed):
    """packed Q (m, H, k), K (n, H, k), V (n, H, d), dO (m, H, d)"""
    rng = np.random.default_rng([seed, heads, k, d, 64 if dtype == np.float64 else 32])
    return (_uniform(rng, (mat.m, heads, k), dtype).mul_(2), _uniform(rng, (mat.n, heads, k), dtype),
            _uniform(rng, (mat.n, heads, d), dtype), _uniform(rng, (mat.m, heads, d), dtype))


def _mha(A, Q, K, V):
    O = torch.full((Q.shape[0],) + tuple(V.shape[1:]), float("nan"), dtype=V.dtype, device=DEV)
    assert A.mha(Q, K, V, O) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return O


def _per_head(A, Q, K, V):
    """the single-head call on every head's slices of the packed tensors, into a packed NaN tensor"""
    O = torch.full((Q.shape[0],) + tuple(V.shape[1:]), float("nan"), dtype=V.dtype, device=DEV)
    for h in range(Q.shape[1]):
        assert A.attention(Q[:, h], K[:, h], V[:, h], O[:, h]) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return O


def _work(mat, heads, dtype):
    return torch.empty(4 * mat.m * heads, dtype=_tdt(dtype), device=DEV)


def _mha_backward(A, mat, Q, K, V, dO, want=(True, True, True)):
    outs = [torch.full(t.shape, float("nan"), dtype=t.dtype, device=DEV) if w else None for t, w in zip((Q, K, V), want)]
    work = _work(mat, Q.shape[1], np.float64 if Q.dtype == torch.float64 else np.float32) if want[1] or want[2] else None
    assert A.mhaBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return outs


def _per_head_backward(A, mat, Q, K, V, dO):
    outs = [torch.full(t.shape, float("nan"), dtype=t.dtype, device=DEV) for t in (Q, K, V)]
    work = torch.empty(4 * mat.m, dtype=Q.dtype, device=DEV)
    for h in range(Q.shape[1]):
        assert A.attentionBackward(Q[:, h], K[:, h], V[:, h], dO[:, h], outs[0][:, h], outs[1][:, h], outs[2][:, h], work) == 0, \
            _capi.last_error()
    torch.cuda.synchronize()
    return outs


def _same(a, b):
    return np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))


# ---- 1. head h equals the single-head call ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", NAMES)
def test_every_head_has_the_bits_of_the_single_head_call(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, dtype)
    for si, (heads, k, d) in enumerate(_shapes(dtype)):
        Q, K, V, _ = _operands(mat, heads, k, d, dtype, seed=100 + si)
        O = _mha(A, Q, K, V)
        assert not bool(torch.isnan(O).any()), (name, heads, k, d, "an element was not written")
        assert _same(O, _per_head(A, Q, K, V)), (name, heads, k, d)
    _close(A)


# ---- 2. the float64 reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_every_head_matches_the_float64_reference(dtype):
    for mi, name in enumerate(("half-empty", "hub", "duplicates")):
        mat = _zoo()[name]
        rows, cols = _index(mat)
        Q, K, V, _ = _operands(mat, 3, 8, 16, dtype, seed=200 + mi)
        A = _open(mat, dtype)
        O = _mha(A, Q, K, V)
        _close(A)
        for h in range(3):
            q, k_, v = Q[:, h].contiguous(), K[:, h].contiguous(), V[:, h].contiguous()
            dY = torch.zeros((mat.m, 16), dtype=_tdt(dtype), device=DEV)
            want = _reference(mat, rows, cols, q, k_, v, dY)[0]
            rho, a_out = _allowances(mat, rows, cols, q, k_, v, dY, dtype)[:2]
            print(f"{name} {_dt(dtype)} head {h}: rho {rho:.3e}")
            assert rho <= RHO_MAX, (name, h, rho)
            _within(O[:, h], want, a_out, f"{name} {_dt(dtype)} head {h}")


# ---- 3. guard --------------------------------------------------------------------------------------------------------------------
def _guarded(rows, width, dtype, guard=64, extra=3):
    """(buffer, view (rows, width) with leading dimension width + extra inside it)"""
    ld = width + extra
    buf = torch.full((guard + rows * ld + guard,), POISON, dtype=_tdt(dtype), device=DEV)
    return buf, buf[guard:guard + rows * ld].view(rows, ld)[:, :width], ld


def _guard_intact(buf, rows, width, ld, guard=64):
    whole = buf.cpu().numpy()
    body = whole[guard:guard + rows * ld].reshape(rows, ld)
    assert (whole[:guard] == POISON).all() and (whole[-guard:] == POISON).all() and (body[:, width:] == POISON).all()
    assert not (body[:, :width] == POISON).any()
    return body[:, :width]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_nothing_but_the_heads_times_width_columns_is_written(dtype):
    heads, k, d = 3, 3, 5
    for name in ("half-empty", "aligned64", "aligned1024"):
        mat = _zoo()[name]
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=31)
        keep = [t.clone() for t in (Q, K, V, dO)]
        A = _open(mat, dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        buf, O2, ldo = _guarded(mat.m, heads * d, dtype)
        O = O2.unflatten(1, (heads, d))
        assert O.stride() == (heads * d + 3, d, 1)
        assert A.mha(Q, K, V, O) == 0, _capi.last_error()
        torch.cuda.synchronize()
        body = _guard_intact(buf, mat.m, heads * d, ldo)
        assert np.array_equal(_bits(body), _bits(_per_head(A, Q, K, V).reshape(mat.m, -1).cpu().numpy())), name
        bufs = [_guarded(t.shape[0], heads * w, dtype) for t, w in ((Q, k), (K, k), (V, d))]
        outs = [b[1].unflatten(1, (heads, w)) for b, w in zip(bufs, (k, k, d))]
        assert A.mhaBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, heads, dtype)) == 0, _capi.last_error()
        torch.cuda.synchronize()
        want = _per_head_backward(A, mat, Q, K, V, dO)
        for (b, _, ld), t, w, g in zip(bufs, (Q, K, V), (k, k, d), want):
            body = _guard_intact(b, t.shape[0], heads * w, ld)
            assert np.array_equal(_bits(body), _bits(g.reshape(t.shape[0], -1).cpu().numpy())), name
        for t, k0 in zip((Q, K, V, dO), keep):
            assert torch.equal(t, k0)
        _close(A)


# ---- 4. the same bits across sigma and paths -------------------------------------------------------------------------------------
SIGMA_PATHS = [Path(f"sigma{s}", s, H.SPMV_FUSED) for s in (4, 7, 32)] + [BY_NAME["fused-default"], BY_NAME["slabs8"]]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_same_bits_on_every_sigma_and_path(dtype):
    for name in ("half-empty", "aligned1024"):
        mat = _zoo()[name]
        Q, K, V, dO = _operands(mat, 3, 8, 16, dtype, seed=41)
        first = None
        for path in SIGMA_PATHS:
            A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), path, dtype)
            assert A.buildTranspose() == 0, _capi.last_error()
            got = [_mha(A, Q, K, V)] + _mha_backward(A, mat, Q, K, V, dO)
            _close(A)
            first = got if first is None else first
            for g, g0 in zip(got, first):
                assert _same(g, g0), (name, path.name)


# ---- 5. the handle is untouched --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_handle_is_untouched(dtype):
    mat = _zoo()["half-empty"]
    rng = np.random.default_rng(51)
    val = rng.uniform(-1, 1, size=mat.nnz).astype(dtype)
    A, _ = _handle(mat, val, BY_NAME["fused-default"], dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    x = _uniform(rng, (mat.n,), dtype)

    def spmv():
        y = torch.full((mat.m,), 3.0, dtype=_tdt(dtype), device=DEV)
        assert A.setX(x) == 0 and A.spmv(1.0, y) == 0
        torch.cuda.synchronize()
        return _bits(y.cpu().numpy())
    y0, info0 = spmv(), bytes(A.info())
    Q, K, V, dO = _operands(mat, 3, 8, 16, dtype, seed=52)
    _mha(A, Q, K, V)
    assert bytes(A.info()) == info0 and np.array_equal(spmv(), y0)
    _mha_backward(A, mat, Q, K, V, dO)
    assert bytes(A.info()) == info0 and np.array_equal(spmv(), y0)
    _close(A)


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_first_calls_are_captured_in_a_graph(dtype):
    """the very first mha and mhaBackward of the handle are the captured ones: enqueue-only from the first call on"""
    mat = _zoo()["half-empty"]
    A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=61)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    outs = [torch.full(t.shape, POISON, dtype=t.dtype, device=DEV) for t in (Q, K, V)]
    work = _work(mat, 3, dtype)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.mha(Q, K, V, O) == 0, _capi.last_error()
        assert A.mhaBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    Qn = _operands(mat, 3, 5, 6, dtype, seed=62)[0]
    Q.copy_(Qn)  # changed in place: the graph reads the same address
    for t in [O] + outs:
        t.fill_(POISON)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in [O] + outs]
    del graph
    assert A.setStream(None) == 0
    eager = [_mha(A, Qn, K, V)] + _mha_backward(A, mat, Qn, K, V, dO)
    for g, e in zip(replayed, eager):
        assert _same(g, e)
    _close(A)


# ---- 7. degenerate cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_no_heads_and_no_columns_are_no_ops_and_k_zero_gives_the_single_head_means(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, dtype)
    Q, K, V, _ = _operands(mat, 3, 4, 6, dtype, seed=71)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    assert A.mha_ptr(0, Q, 12, K, 12, 4, V, 18, 6, O, 18) == 0, _capi.last_error()  # heads = 0
    assert A.mha_ptr(3, Q, 12, K, 12, 4, V, 18, 0, O, 18) == 0, _capi.last_error()  # d = 0
    empty = torch.zeros((mat.m, 0, 6), dtype=_tdt(dtype), device=DEV)
    assert A.mha(torch.zeros((mat.m, 0, 4), dtype=_tdt(dtype), device=DEV), torch.zeros((mat.n, 0, 4), dtype=_tdt(dtype), device=DEV),
                 torch.zeros((mat.n, 0, 6), dtype=_tdt(dtype), device=DEV), empty) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert bool((O == POISON).all())
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))  # k = 0: per-head row means
    got = _mha(A, Q0, K0, V)
    assert not bool(torch.isnan(got).any()) and _same(got, _per_head(A, Q0, K0, V))
    _close(A)
    none = zoo.empty_matrix()
    A = _open(none, dtype)
    Q, K, V, _ = _operands(none, 3, 4, 6, dtype, seed=72)
    assert not _bits(_mha(A, Q, K, V).cpu().numpy()).any()  # +0 everywhere
    _close(A)


# ---- 8. non-finite values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_nan_in_one_head_of_one_row_stays_there(dtype):
    mat = S.duplicates_matrix()
    lens = np.diff(mat.row_ptr)
    b = int(np.flatnonzero(lens >= 2)[0])
    Q, K, V, _ = _operands(mat, 3, 4, 6, dtype, seed=81)
    A = _open(mat, dtype)
    benign = _mha(A, Q, K, V)
    bad = Q.clone()
    bad[b, 1, 1] = float("nan")
    O = _mha(A, bad, K, V)
    _close(A)
    assert bool(torch.isnan(O[b, 1]).all())
    mask = torch.ones((mat.m, 3), dtype=torch.bool, device=DEV)
    mask[b, 1] = False
    assert not bool(torch.isnan(O[mask]).any()) and _same(O[mask], benign[mask])


# ---- 9. backward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("half-empty", "aligned64", "two-hubs", "duplicates"))
def test_backward_has_the_bits_of_the_single_head_backward(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, dtype)
    alone = []
    for si, (heads, k, d) in enumerate(((2, 8, 16), (3, 3, 5))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=90 + si)
        alone.append(_mha_backward(A, mat, Q, K, V, dO, want=(True, False, False))[0])  # neither workspace nor companion
        assert A.info().transpose_built == 0
        assert A.mhaBackward(Q, K, V, dO, None, torch.empty_like(K), None, _work(mat, heads, dtype)) != 0  # no companion
        assert "transposed companion" in _capi.last_error()
    assert A.buildTranspose() == 0, _capi.last_error()  # (only now: the calls above ran without it)
    for si, (heads, k, d) in enumerate(((2, 8, 16), (3, 3, 5))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=90 + si)
        full = _mha_backward(A, mat, Q, K, V, dO)
        assert _same(alone[si], full[0]), (name, "dQ alone")
        for g, w, what in zip(full, _per_head_backward(A, mat, Q, K, V, dO), ("dQ", "dK", "dV")):
            assert not bool(torch.isnan(g).any()), (name, what, "an element was not written")
            assert _same(g, w), (name, heads, k, d, what)
        for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True),
                     (False, True, True)):
            for g, g0, w in zip(_mha_backward(A, mat, Q, K, V, dO, want=want), full, want):
                assert (g is None) == (not w)
                assert g is None or _same(g, g0), (name, want)
    _close(A)


# ---- 10. autograd ----------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_multihead_attention():
    """fp64, torch's default tolerances, on the matrix with repeated pairs and empty rows at sigma = 4; clones as in
    tests/test_gpu_fused_attention.py (gradcheck perturbs through ``.data``)"""
    mat = S.duplicates_matrix()
    A = _open(mat, np.float64, sigma=4)
    rng = np.random.default_rng(3)
    Q = _uniform(rng, (mat.m, 2, 3), np.float64).requires_grad_(True)
    K = _uniform(rng, (mat.n, 2, 3), np.float64).requires_grad_(True)
    V = _uniform(rng, (mat.n, 2, 2), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q, k, v: autograd.multihead_attention(A, q.clone(), k.clone(), v.clone()), (Q, K, V))
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_gradients_equal_those_of_fused_attention_per_head(dtype):
    for mi, name in enumerate(("half-empty", "hub")):
        mat = _zoo()[name]
        Q, K, V, dO = _operands(mat, 3, 8, 5, dtype, seed=110 + mi)
        A = _open(mat, dtype)
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        out = autograd.multihead_attention(A, q, k, v)
        out.backward(dO)
        torch.cuda.synchronize()
        heads = []
        for h in range(3):
            qh, kh, vh = (t[:, h].clone().requires_grad_(True) for t in (Q, K, V))
            oh = autograd.fused_attention(A, qh, kh, vh, backward="fused")
            oh.backward(dO[:, h])
            heads.append((oh.detach(), qh.grad, kh.grad, vh.grad))
        torch.cuda.synchronize()
        _close(A)
        for got, i in zip((out.detach(), q.grad, k.grad, v.grad), range(4)):
            assert _same(got, torch.stack([hd[i] for hd in heads], dim=1)), (name, i)


def test_forward_without_gradients_leaves_the_handle_alone():
    mat = S.duplicates_matrix()
    A, _ = _handle(mat, np.ones(mat.nnz), BY_NAME["fused-default"], np.float64)
    Q, K, V, dO = _operands(mat, 2, 3, 2, np.float64, seed=120)
    with torch.no_grad():
        out = autograd.multihead_attention(A, Q, K, V)
    torch.cuda.synchronize()
    assert not out.requires_grad and getattr(A, "_autograd_key", None) is None and A.info().transpose_built == 0
    q = Q.clone().requires_grad_(True)
    autograd.multihead_attention(A, q, K, V).backward(dO)
    torch.cuda.synchronize()
    assert q.grad is not None and A.info().transpose_built == 0 and getattr(A, "_autograd_key", None) is None  # dQ alone
    _close(A)
