"""csr5hip_attention (``A.attention``) and ``autograd.fused_attention`` on the GPU: the output against the float64 torch reference
within the bound derived in tests/test_gpu_attention_autograd.py (it holds for any summation order and for either placement of
the normalisation), the same bits on every layout, leading dimension and alignment, untouched guard bytes and an untouched
handle, special values, graph capture, and the autograd wrapper (gradcheck, gradients equal to ``autograd.attention``'s).

Row classes of the kernel and where they are met: at most 16 entries (kat0, half-empty, ...), 17 .. 512 (aligned64, row 5 of the
duplicates matrix), 513 .. 2 048 (aligned1024) and beyond (hub, two-hubs, one-row); d = 70 has a second column block of 6
columns, d = 300 (the wide test) a second group of four blocks.  None of these rows sits ON a class edge and every row beyond 512
entries lies in workgroup 0: the edges (17, 63 | 64 | 65, 511 | 512 | 513, 2 048 | 2 049, 4 096 | 4 097), hubs in later
workgroups, second column blocks of width 1 and the output bit for bit are in tests/test_gpu_attention_edges.py."""
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
from tests.test_gpu_attention_autograd import _allowances, _index, _open, _reference, _uniform, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, Path, _bits, _close, _handle  # noqa: E402

NAMES = ("kat0", "tiny-p1", "dense16", "nonsquare", "half-empty", "hub", "aligned64", "aligned1024", "two-hubs", "one-row",
         "single-nnz")
KD = ((1, 1), (3, 5), (8, 16), (13, 64), (40, 70))
RHO_MAX = 2.0 ** -6
POISON = -777.25
BY_NAME = {p.name: p for p in PATHS}


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


@functools.lru_cache(maxsize=1)
def _zoo():
    return {m.name: m for m in zoo.small_zoo()}


def _matrices():
    return [_zoo()[n] for n in NAMES] + [S.duplicates_matrix()]


def _operands(mat, k, d, dtype, seed):
    rng = np.random.default_rng([seed, k, d, 64 if dtype == np.float64 else 32])
    return _uniform(rng, (mat.m, k), dtype).mul_(2), _uniform(rng, (mat.n, k), dtype), _uniform(rng, (mat.n, d), dtype)


def _attend(A, Q, K, V):
    """A.attention into a poisoned O: every element must be written"""
    O = torch.full((Q.shape[0], V.shape[1]), float("nan"), dtype=V.dtype, device=DEV)
    assert A.attention(Q, K, V, O) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return O


def _empty_rows(mat):
    return torch.from_numpy(np.diff(mat.row_ptr) == 0).to(DEV)


def _bound(mat, Q, K, V, dtype):
    rows, cols = _index(mat)
    dY = torch.zeros((mat.m, V.shape[1]), dtype=V.dtype, device=DEV)
    want = _reference(mat, rows, cols, Q, K, V, dY)[0]
    rho, a_out = _allowances(mat, rows, cols, Q, K, V, dY, dtype)[:2]
    return want, rho, a_out


# ---- 1. accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("kd", KD, ids=lambda kd: f"k{kd[0]}-d{kd[1]}")
def test_output_matches_the_float64_reference(kd, dtype):
    k, d = kd
    for mi, mat in enumerate(_matrices()):
        Q, K, V = _operands(mat, k, d, dtype, seed=100 + mi)
        A = _open(mat, dtype)
        O = _attend(A, Q, K, V)
        want, rho, a_out = _bound(mat, Q, K, V, dtype)
        print(f"{mat.name} {_dt(dtype)} k={k} d={d}: rho {rho:.3e}")
        assert rho <= RHO_MAX, (mat.name, rho)
        _within(O, want, a_out, f"{mat.name} {_dt(dtype)} k={k} d={d}")
        empty = _empty_rows(mat)
        assert not _bits(O[empty].cpu().numpy()).any(), mat.name  # rows without entries: exactly +0
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_more_than_four_column_blocks(dtype):
    """d = 300: rows beyond 512 entries sweep the columns in groups of 256 (and recompute their scores beyond 2 048 entries)"""
    for mi, name in enumerate(("aligned1024", "one-row", "kat0")):
        mat = _zoo()[name]
        Q, K, V = _operands(mat, 5, 300, dtype, seed=300 + mi)
        A = _open(mat, dtype)
        O = _attend(A, Q, K, V)
        want, rho, a_out = _bound(mat, Q, K, V, dtype)
        assert rho <= RHO_MAX, (mat.name, rho)
        _within(O, want, a_out, f"{mat.name} {_dt(dtype)} d=300")
        _close(A)


# ---- 2. the same bits on every layout ------------------------------------------------------------------------------------------
LAYOUT_NAMES = ("half-empty", "hub", "aligned1024")


@functools.lru_cache(maxsize=None)
def _default_bits(name, dtype):
    mat = _zoo()[name]
    Q, K, V = _operands(mat, 8, 16, dtype, seed=7)
    A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
    O = _attend(A, Q, K, V).cpu().numpy()
    _close(A)
    return _bits(O)


SIGMA_PATHS = [Path(f"sigma{s}", s, H.SPMV_FUSED) for s in (4, 7, 16, 32)]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("path", PATHS + SIGMA_PATHS, ids=lambda p: p.name)
def test_same_bits_on_every_path_and_sigma(path, dtype):
    for name in LAYOUT_NAMES:
        mat = _zoo()[name]
        Q, K, V = _operands(mat, 8, 16, dtype, seed=7)
        A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), path, dtype)
        O = _attend(A, Q, K, V).cpu().numpy()
        _close(A)
        assert np.array_equal(_bits(O), _default_bits(name, dtype)), (path.name, name)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_same_bits_for_column_slices_and_offset_pointers(dtype):
    """(k, d) = (8, 16): the contiguous operands take 16-byte loads; slices of wider tensors with odd leading dimensions and
    pointers one element into an allocation take element loads -- the same chains, the same bits"""
    for name in LAYOUT_NAMES:
        mat = _zoo()[name]
        Q, K, V = _operands(mat, 8, 16, dtype, seed=7)
        A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)

        def sliced(t, pad_left, pad_right):
            wide = torch.full((t.shape[0], pad_left + t.shape[1] + pad_right), POISON, dtype=t.dtype, device=DEV)
            wide[:, pad_left:pad_left + t.shape[1]] = t
            return wide[:, pad_left:pad_left + t.shape[1]]

        def offset(t):
            flat = torch.full((t.numel() + 1,), POISON, dtype=t.dtype, device=DEV)
            flat[1:] = t.reshape(-1)
            return flat[1:].view(t.shape)
        Os = torch.full((mat.m, 16 + 5), POISON, dtype=_tdt(dtype), device=DEV)
        assert A.attention(sliced(Q, 3, 2), sliced(K, 1, 0), sliced(V, 0, 7), Os[:, 2:18]) == 0, _capi.last_error()
        Oo = offset(torch.zeros((mat.m, 16), dtype=_tdt(dtype), device=DEV))
        assert A.attention(offset(Q), offset(K), offset(V), Oo) == 0, _capi.last_error()
        # heads as column slices: two heads of one wide tensor, each equal to a call on its own copy
        Q2, K2, V2 = _operands(mat, 16, 32, dtype, seed=8)
        O2 = torch.full((mat.m, 32), POISON, dtype=_tdt(dtype), device=DEV)
        for h in range(2):
            assert A.attention(Q2[:, 8 * h:8 * h + 8], K2[:, 8 * h:8 * h + 8], V2[:, 16 * h:16 * h + 16],
                               O2[:, 16 * h:16 * h + 16]) == 0, _capi.last_error()
        heads = [_attend(A, Q2[:, 8 * h:8 * h + 8].contiguous(), K2[:, 8 * h:8 * h + 8].contiguous(),
                         V2[:, 16 * h:16 * h + 16].contiguous()) for h in range(2)]
        torch.cuda.synchronize()
        _close(A)
        want = _default_bits(name, dtype)
        assert np.array_equal(_bits(Os[:, 2:18].cpu().numpy()), want), name
        assert np.array_equal(_bits(Oo.cpu().numpy()), want), name
        assert bool((Os[:, :2] == POISON).all()) and bool((Os[:, 18:] == POISON).all())
        assert np.array_equal(_bits(O2.cpu().numpy()), _bits(torch.cat(heads, dim=1).cpu().numpy())), name


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_row_alone_gives_the_bits_it_has_inside_a_matrix(dtype):
    mat = _zoo()["two-hubs"]
    Q, K, V = _operands(mat, 8, 16, dtype, seed=9)
    A = _open(mat, dtype)
    O = _attend(A, Q, K, V).cpu().numpy()
    _close(A)
    for r in (0, 3, 8):  # 5 000, 7 000 and 2 entries
        a, b = int(mat.row_ptr[r]), int(mat.row_ptr[r + 1])
        one = M.CsrMatrix(1, mat.n, np.array([0, b - a], dtype=np.int32), mat.col[a:b].copy(), np.ones(b - a), f"row{r}")
        A1 = _open(one, dtype, sigma=7)
        O1 = _attend(A1, Q[r:r + 1].clone(), K, V).cpu().numpy()
        _close(A1)
        assert np.array_equal(_bits(O1[0]), _bits(O[r])), r


# ---- 3. poison and guard -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_nothing_but_the_d_columns_is_written(dtype):
    for name in ("half-empty", "hub", "aligned64"):
        mat = _zoo()[name]
        d, ldo, guard = 5, 8, 64
        Q, K, V = _operands(mat, 3, d, dtype, seed=11)
        keep = [t.clone() for t in (Q, K, V)]
        buf = torch.full((guard + mat.m * ldo + guard,), POISON, dtype=_tdt(dtype), device=DEV)
        O = buf[guard:guard + mat.m * ldo].view(mat.m, ldo)[:, :d]
        assert O.stride(0) == ldo == d + 3
        A = _open(mat, dtype)
        assert A.attention(Q, K, V, O) == 0, _capi.last_error()
        torch.cuda.synchronize()
        _close(A)
        whole = buf.cpu().numpy()
        body = whole[guard:guard + mat.m * ldo].reshape(mat.m, ldo)
        assert (whole[:guard] == POISON).all() and (whole[-guard:] == POISON).all() and (body[:, d:] == POISON).all()
        assert not (body[:, :d] == POISON).any()
        want, rho, a_out = _bound(mat, Q, K, V, dtype)
        _within(O, want, a_out, f"{name} strided O")
        for t, k0 in zip((Q, K, V), keep):
            assert torch.equal(t, k0)


# ---- 4. the handle is untouched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_handle_is_untouched(dtype):
    mat = _zoo()["half-empty"]
    rng = np.random.default_rng(12)
    val = rng.uniform(-1, 1, size=mat.nnz).astype(dtype)
    A, _ = _handle(mat, val, BY_NAME["fused-default"], dtype)
    x = _uniform(rng, (mat.n,), dtype)

    def spmv():
        y = torch.full((mat.m,), 3.0, dtype=_tdt(dtype), device=DEV)
        assert A.setX(x) == 0 and A.spmv(1.0, y) == 0
        torch.cuda.synchronize()
        return _bits(y.cpu().numpy())
    y0, info0 = spmv(), bytes(A.info())
    Q, K, V = _operands(mat, 8, 16, dtype, seed=13)
    _attend(A, Q, K, V)
    assert bytes(A.info()) == info0 and A.info().transpose_built == 0
    assert np.array_equal(spmv(), y0)
    _close(A)


# ---- 5. special values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_k_zero_gives_row_means_and_d_zero_is_a_no_op(dtype):
    u = unit_roundoff(dtype)
    for name in ("half-empty", "hub", "aligned64"):
        mat = _zoo()[name]
        rows, cols = _index(mat)
        _, _, V = _operands(mat, 1, 7, dtype, seed=14)
        A = _open(mat, dtype)
        O = _attend(A, torch.zeros((mat.m, 0), dtype=_tdt(dtype), device=DEV), torch.zeros((mat.n, 0), dtype=_tdt(dtype), device=DEV), V)
        L = torch.from_numpy(np.diff(mat.row_ptr).astype(np.float64)).to(DEV)
        sums = torch.zeros((mat.m, 7), dtype=torch.float64, device=DEV).index_add(0, rows, V.double()[cols])
        sabs = torch.zeros((mat.m, 7), dtype=torch.float64, device=DEV).index_add(0, rows, V.double()[cols].abs())
        Lc = L.clamp_min(1)[:, None]
        # w = 1 and Z = L exactly; a chain or tree of L terms, one reciprocal, one product: gamma(L + 2) of the mean of |V|
        n = L[:, None] + 2
        allowed = (n * u / (1 - n * u)) * sabs / Lc * (2 if dtype == np.float64 else 1 + 2.0 ** -10)
        _within(O, sums / Lc, allowed, f"{name} k = 0")
        assert not _bits(O[_empty_rows(mat)].cpu().numpy()).any()
        Q, K, _ = _operands(mat, 4, 1, dtype, seed=15)
        assert A.attention(Q, K, torch.zeros((mat.n, 0), dtype=_tdt(dtype), device=DEV),
                           torch.zeros((mat.m, 0), dtype=_tdt(dtype), device=DEV)) == 0
        assert A.attention_ptr(Q, 4, K, 4, 4, None, 0, 0, None, 0) == 0
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_matrix_without_entries_gives_zeros(dtype):
    mat = zoo.empty_matrix()
    A = _open(mat, dtype)
    Q, K, V = _operands(mat, 4, 6, dtype, seed=16)
    O = _attend(A, Q, K, V)
    assert O.shape == (mat.m, 6) and not _bits(O.cpu().numpy()).any()
    O.fill_(POISON)
    assert A.attention_ptr(None, 4, None, 4, 4, None, 6, 6, O, 6) == 0  # nnz = 0: only O is needed
    torch.cuda.synchronize()
    assert not _bits(O.cpu().numpy()).any()
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_non_finite_scores_stay_in_their_rows(dtype):
    """Q[a, 0] = -huge against K[:, 0] in {0, 2}: the entries of row a whose column has 2 overflow to -Inf (weight +0), the
    others are finite; row c has 2 in all its columns (only -Inf: NaN); row b has a NaN in Q (NaN).  Every other row is within
    the bound."""
    mat = S.duplicates_matrix()
    lens = np.diff(mat.row_ptr)
    rows_np = S.rows_of(mat)
    huge = -1e308 if dtype == np.float64 else -3e38
    c = int(np.flatnonzero(lens == 3)[0])
    cols_c = set(mat.col[mat.row_ptr[c]:mat.row_ptr[c + 1]].tolist())
    a = next(int(r) for r in np.flatnonzero(lens >= 6) if r != c and
             len(set(mat.col[mat.row_ptr[r]:mat.row_ptr[r + 1]].tolist()) - cols_c) >= 3)
    cols_a = mat.col[mat.row_ptr[a]:mat.row_ptr[a + 1]]
    free = sorted(set(cols_a.tolist()) - cols_c)
    b = next(int(r) for r in np.flatnonzero(lens >= 2) if r not in (a, c))
    Q, K, V = _operands(mat, 4, 6, dtype, seed=17)
    K[:, 0] = 0
    K[torch.tensor(sorted(cols_c) + free[:1], device=DEV), 0] = 2
    benign = Q.clone()
    benign[a, 0] = 0
    benign[c, 0] = 0
    want, rho, a_out = _bound(mat, benign, K, V, dtype)
    Q[a, 0] = huge
    Q[c, 0] = huge
    Q[b, 1] = float("nan")
    A = _open(mat, dtype)
    O = _attend(A, Q, K, V)
    _close(A)
    assert bool(torch.isnan(O[b]).all()) and bool(torch.isnan(O[c]).all())
    others = torch.ones(mat.m, dtype=torch.bool, device=DEV)
    others[[a, b, c]] = False
    assert bool(torch.isfinite(O[others]).all())
    _within(O[others], want[others], a_out[others], "rows beside the non-finite ones")
    # row a: the softmax over the entries whose K[:, 0] is 0 (Q[a, 0] * 0 adds a zero to their chains)
    kept = torch.from_numpy(cols_a.astype(np.int64)).to(DEV)
    kept = kept[K[kept, 0] == 0]
    assert 0 < kept.numel() < cols_a.size
    p = torch.softmax((benign[a].double()[None, :] * K.double()[kept]).sum(dim=1), dim=0)
    _within(O[a], (p[:, None] * V.double()[kept]).sum(dim=0), rho * (p[:, None] * V.double()[kept].abs()).sum(dim=0), "masked row")
    assert rows_np.size == mat.nnz


# ---- 6. graph capture ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_attention_is_captured_in_a_graph(dtype):
    """one kernel on the handle's stream; the very first attention of the handle is the captured one (enqueue-only from the
    first call: a host synchronisation or an allocation inside the call would break the capture)"""
    mat = _zoo()["half-empty"]
    A, _ = _handle(mat, np.ones(mat.nnz, dtype=dtype), BY_NAME["fused-default"], dtype)
    Q, K, V = _operands(mat, 13, 20, dtype, seed=18)
    O = torch.full((mat.m, 20), POISON, dtype=_tdt(dtype), device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.attention(Q, K, V, O) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    replayed = []
    news = [_operands(mat, 13, 20, dtype, seed=19 + i)[0] for i in range(2)]
    for Qn in news:
        Q.copy_(Qn)  # changed in place: the graph reads the same address
        O.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replayed.append(O.cpu().numpy().copy())
    del graph
    assert A.setStream(None) == 0
    for Qn, got in zip(news, replayed):
        assert np.array_equal(_bits(_attend(A, Qn, K, V).cpu().numpy()), _bits(got))
    assert not np.array_equal(replayed[0], replayed[1])
    _close(A)


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------
def test_gradcheck_of_fused_attention():
    """fp64, torch's default tolerances, on the matrix with repeated pairs and empty rows at sigma = 4 (p >= 2); clones as in
    tests/test_gpu_attention_autograd.py (gradcheck perturbs through ``.data``)"""
    mat = S.duplicates_matrix()
    A = _open(mat, np.float64, sigma=4)
    assert A.info().p >= 2 and (np.diff(mat.row_ptr) == 0).any()
    rng = np.random.default_rng(3)
    Q = _uniform(rng, (mat.m, 3), np.float64).requires_grad_(True)
    K = _uniform(rng, (mat.n, 3), np.float64).requires_grad_(True)
    V = _uniform(rng, (mat.n, 2), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q, k, v: autograd.fused_attention(A, q.clone(), k.clone(), v.clone()), (Q, K, V))
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_gradients_equal_those_of_the_unfused_attention(dtype):
    rng = np.random.default_rng(21)
    for mat in (_zoo()["half-empty"], _zoo()["hub"], S.duplicates_matrix()):
        rows, cols = _index(mat)
        Q = _uniform(rng, (mat.m, 8), dtype).mul_(2)
        K, V = _uniform(rng, (mat.n, 8), dtype), _uniform(rng, (mat.n, 5), dtype)
        dY = _uniform(rng, (mat.m, 5), dtype)
        got = []
        for fn in (autograd.fused_attention, autograd.attention):
            A = _open(mat, dtype)
            q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
            out = fn(A, q, k, v)
            out.backward(dY)
            torch.cuda.synchronize()
            got.append((out.detach(), q.grad, k.grad, v.grad))
            _close(A)
        for f, u_ in zip(got[0][1:], got[1][1:]):
            assert torch.equal(f, u_), mat.name
        want = _reference(mat, rows, cols, Q, K, V, dY)[0]
        rho, a_out = _allowances(mat, rows, cols, Q, K, V, dY, dtype)[:2]
        assert rho <= RHO_MAX
        _within(got[0][0], want, a_out, f"{mat.name} {_dt(dtype)} fused out")


def test_forward_without_gradients_leaves_the_handle_alone_and_q_alone_needs_no_companion():
    mat = S.duplicates_matrix()
    rng = np.random.default_rng(22)
    val = rng.uniform(-1, 1, size=mat.nnz)
    A, _ = _handle(mat, val, BY_NAME["fused-default"], np.float64)
    x = _uniform(rng, (mat.n,), np.float64)

    def spmv():
        y = torch.full((mat.m,), 3.0, dtype=torch.float64, device=DEV)
        assert A.setX(x) == 0 and A.spmv(1.0, y) == 0
        torch.cuda.synchronize()
        return _bits(y.cpu().numpy())
    y0 = spmv()
    Q, K, V = _uniform(rng, (mat.m, 3), np.float64), _uniform(rng, (mat.n, 3), np.float64), _uniform(rng, (mat.n, 2), np.float64)
    with torch.no_grad():
        out = autograd.fused_attention(A, Q, K, V)
    torch.cuda.synchronize()
    assert not out.requires_grad and getattr(A, "_autograd_key", None) is None
    assert np.array_equal(spmv(), y0) and A.info().transpose_built == 0
    # a forward that will be differentiated touches no more
    q = Q.clone().requires_grad_(True)
    out = autograd.fused_attention(A, q, K, V)
    torch.cuda.synchronize()
    assert getattr(A, "_autograd_key", None) is None and np.array_equal(spmv(), y0)
    dY = _uniform(rng, (mat.m, 2), np.float64)
    out.backward(dY)
    torch.cuda.synchronize()
    assert A.info().transpose_built == 0  # a gradient for Q alone
    rows, cols = _index(mat)
    _, rQ, _, _ = _reference(mat, rows, cols, Q, K, V, dY)
    a_Q = _allowances(mat, rows, cols, Q, K, V, dY, np.float64)[2]
    _within(q.grad, rQ, a_Q, "dQ alone")
    k = K.clone().requires_grad_(True)
    autograd.fused_attention(A, Q, k, V).backward(dY)
    assert A.info().transpose_built == 1 and k.grad is not None
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_fused_attention_on_a_side_stream_gives_the_same_bits(dtype):
    mat = _zoo()["half-empty"]
    rng = np.random.default_rng(23)
    A = _open(mat, dtype)
    Q, K, V = _uniform(rng, (mat.m, 5), dtype), _uniform(rng, (mat.n, 5), dtype), _uniform(rng, (mat.n, 4), dtype)
    dY = _uniform(rng, (mat.m, 4), dtype)

    def run():
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        out = autograd.fused_attention(A, q, k, v)
        out.backward(dY)
        return out.detach(), q.grad, k.grad, v.grad
    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    torch.cuda.synchronize()
    third = run()
    torch.cuda.synchronize()
    for x, y, z in zip(first, second, third):
        assert torch.equal(x, y) and torch.equal(x, z)
    _close(A)
