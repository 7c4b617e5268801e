"""autograd.row_softmax, autograd.sddmm and autograd.attention on the GPU: gradcheck, agreement of the attention product and its
three gradients with a torch reference built from a row index, two forwards before either backward on one handle, the companion
built only when K or V needs a gradient, and a non-default stream.

THE BOUND of ``test_attention_matches_a_torch_reference``.  The reference runs the same expression in torch in float64 from a
row index (scatter_reduce / index_add; repeated (row, column) pairs stay separate entries).  With u the unit roundoff of the
tested precision, k the width of Q and K, L the length of a row and gamma(n) = n u / (1 - n u):

* a score is a chain of k fused multiply-adds: |ds_e| <= gamma(k) sum_c |Q[i, c] K[j, c]| =: sigma_e (Higham section 4.2);
* a softmax whose scores move by at most sigma = max_row sigma_e moves by at most the relative 2 sigma (numerator and
  denominator each by at most e**sigma), and the kernel adds the relative forward bound of tests/softmax_reference.py,
  beta_e = u [(|d_e| + c) + sum_j p_j (|d_j| + c)] (1 + 2**-10) + gamma(L - 1) + 2 u;
* the product sums L terms p V: gamma(L) on each.

So every output carries at most the relative error rho = max over the matrix of (2 sigma + beta + gamma(L)) on each of its
terms, and  |out - ref|[i, c] <= rho sum_j p_ij |V[j, c]|  -- the forward bound propagated through the product.  The gradients
are sums of products of at most STAGES = 8 such factors and sums (dY, p, V; the softmax gradient's product, sum, difference and
product; Q or K; the final sum), each within rho of its exact value, so to first order
|grad - ref| <= STAGES rho A, where A is the same gradient expression evaluated on absolute values (no cancellation):
A_V = sum_i p |dY|, A_p = |dY| . |V|, A_s = p (A_p + sum_row p A_p), A_Q = sum_j A_s |K|, A_K = sum_i A_s |Q|.
The terms this drops are (1 + rho)**STAGES - 1 - STAGES rho <= (STAGES rho)**2 / (2 (1 - STAGES rho)) of A.  The test asserts
STAGES rho <= FIRST_ORDER = 2**-6 before it compares, which keeps them under 1/126 of the allowance; rho is a function of the
inputs alone (not of what the library returns), so this is a condition on the test's data.  The longest row of the suite, the
"hub" matrix's 9000 entries, has 2 gamma(9000) = 1.07e-3 in fp32, STAGES rho = 8.7e-3: a guard below that could never hold.
For fp64 the reference is itself computed in fp64 by the same kind of operations and obeys the same bound: the allowance is
doubled there; for fp32 the float64 reference's error (2**-29 of the allowance) is covered by the factor (1 + 2**-10)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import softmax_reference as R  # noqa: E402
from tests import zoo  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
STAGES = 8
FIRST_ORDER = 2.0 ** -6  # STAGES * rho stays below this: see the module docstring


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _open(mat, dtype, sigma=AUTO):
    return _handle(mat, np.ones(mat.nnz, dtype=dtype), Path("autograd", sigma, H.SPMV_FUSED), dtype)[0]


def _uniform(rng, shape, dtype):
    return torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(dtype)).to(DEV)


def _index(mat):
    rows = torch.from_numpy(S.rows_of(mat)).to(DEV)
    cols = torch.from_numpy(mat.col[:mat.nnz].astype(np.int64)).to(DEV)
    return rows, cols


def _torch_softmax(mat, rows, scores):
    M = torch.full((mat.m,), -float("inf"), dtype=scores.dtype, device=DEV).scatter_reduce(0, rows, scores.detach(), "amax")
    e = torch.exp(scores - M[rows])  # (the softmax does not depend on M: it is a constant of the graph)
    Z = torch.zeros(mat.m, dtype=scores.dtype, device=DEV).index_add(0, rows, e)
    return e / Z[rows]


def _torch_attention(mat, rows, cols, Q, K, V):
    p = _torch_softmax(mat, rows, (Q[rows] * K[cols]).sum(dim=1))
    return torch.zeros((mat.m, V.shape[1]), dtype=V.dtype, device=DEV).index_add(0, rows, p[:, None] * V[cols]), p


def test_gradcheck_of_the_three_functions():
    """fp64, torch's default tolerances, on the matrix with repeated pairs and empty rows at sigma = 4 (p >= 2).  gradcheck
    perturbs its inputs through ``.data``, which does not move ``_version``: the clone hands every evaluation tensors of its
    own, as the module's docstring asks for such writes."""
    mat = S.duplicates_matrix()
    A = _open(mat, np.float64, sigma=4)
    assert A.info().p >= 2 and (np.diff(mat.row_ptr) == 0).any()
    rng = np.random.default_rng(3)
    s = _uniform(rng, mat.nnz, np.float64).mul_(3).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: autograd.row_softmax(A, t.clone()), (s,))
    U = _uniform(rng, (mat.m, 3), np.float64).requires_grad_(True)
    W = _uniform(rng, (mat.n, 3), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: autograd.sddmm(A, a.clone(), b.clone()), (U, W))
    Q = _uniform(rng, (mat.m, 3), np.float64).requires_grad_(True)
    K = _uniform(rng, (mat.n, 3), np.float64).requires_grad_(True)
    V = _uniform(rng, (mat.n, 2), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q, k, v: autograd.attention(A, q.clone(), k.clone(), v.clone()), (Q, K, V))
    _close(A)


def _allowances(mat, rows, cols, Q, K, V, dY, dtype):
    """(rho, forward allowance (m, d), allowances of dQ, dK, dV) in float64 on the device: the module docstring's bound"""
    u = unit_roundoff(dtype)
    k = Q.shape[1]
    Qd, Kd, Vd, dYd = (t.detach().double() for t in (Q, K, V, dY))
    s = (Qd[rows] * Kd[cols]).sum(dim=1)
    sigma = float(((k * u / (1 - k * u)) * (Qd[rows].abs() * Kd[cols].abs()).sum(dim=1)).max())
    ref = R.softmax_reference(mat.row_ptr, s.cpu().numpy().astype(dtype))
    with np.errstate(invalid="ignore", divide="ignore"):
        beta = float(np.nanmax(np.where(ref.expected > 0, ref.bound / ref.expected, 0)))
    Lmax = int(np.diff(mat.row_ptr).max())
    rho = (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * (1 + 2.0 ** -10) * (2 if dtype == np.float64 else 1)
    p = _torch_softmax(mat, rows, s)
    zeros = lambda n, d: torch.zeros((n, d), dtype=torch.float64, device=DEV)  # noqa: E731
    a_out = zeros(mat.m, Vd.shape[1]).index_add(0, rows, p[:, None] * Vd[cols].abs())
    a_V = zeros(mat.n, Vd.shape[1]).index_add(0, cols, p[:, None] * dYd[rows].abs())
    a_p = (dYd[rows].abs() * Vd[cols].abs()).sum(dim=1)
    a_s = p * (a_p + torch.zeros(mat.m, dtype=torch.float64, device=DEV).index_add(0, rows, p * a_p)[rows])
    a_Q = zeros(mat.m, k).index_add(0, rows, a_s[:, None] * Kd[cols].abs())
    a_K = zeros(mat.n, k).index_add(0, cols, a_s[:, None] * Qd[rows].abs())
    return rho, rho * a_out, STAGES * rho * a_Q, STAGES * rho * a_K, STAGES * rho * a_V


def _reference(mat, rows, cols, Q, K, V, dY):
    Qr, Kr, Vr = (t.detach().double().clone().requires_grad_(True) for t in (Q, K, V))
    out, _ = _torch_attention(mat, rows, cols, Qr, Kr, Vr)
    out.backward(dY.double())
    return out.detach(), Qr.grad, Kr.grad, Vr.grad


def _within(got, want, allowed, what):
    err = (got.double() - want).abs()
    worst = float((err / allowed.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst |error| / allowance {worst:.3f}")
    assert bool((err <= allowed).all()), (what, worst)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_attention_matches_a_torch_reference(dtype):
    rng = np.random.default_rng(17)
    for mat in [m for m in zoo.small_zoo() if m.name in ("half-empty", "hub", "nonsquare")] + [S.duplicates_matrix()]:
        rows, cols = _index(mat)
        Q = _uniform(rng, (mat.m, 8), dtype).mul_(2).requires_grad_(True)
        K = _uniform(rng, (mat.n, 8), dtype).requires_grad_(True)
        V = _uniform(rng, (mat.n, 5), dtype).requires_grad_(True)
        dY = _uniform(rng, (mat.m, 5), dtype)
        A = _open(mat, dtype)
        out = autograd.attention(A, Q, K, V)
        out.backward(dY)
        torch.cuda.synchronize()
        want, gQ, gK, gV = _reference(mat, rows, cols, Q, K, V, dY)
        rho, a_out, a_Q, a_K, a_V = _allowances(mat, rows, cols, Q, K, V, dY, dtype)
        assert STAGES * rho <= FIRST_ORDER, (mat.name, rho)
        what = f"{mat.name} {np.dtype(dtype).name}"
        _within(out.detach(), want, a_out, what + " out")
        _within(Q.grad, gQ, a_Q, what + " dQ")
        _within(K.grad, gK, a_K, what + " dK")
        _within(V.grad, gV, a_V, what + " dV")
        empty = torch.from_numpy(np.diff(mat.row_ptr) == 0).to(DEV)
        assert not out.detach()[empty].any() and not Q.grad[empty].any()  # rows without entries: 0 out, 0 gradient
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_two_forwards_before_either_backward(dtype):
    """the second forward leaves its softmax in the handle, the first backward gives the handle a gradient as values (sddmm's
    backward) in between: spmm's backward must give p back to A and A^T before it multiplies"""
    rng = np.random.default_rng(5)
    for mat in [m for m in zoo.small_zoo() if m.name in ("half-empty", "hub")] + [S.duplicates_matrix()]:
        rows, cols = _index(mat)
        A = _open(mat, dtype)
        K = _uniform(rng, (mat.n, 4), dtype).requires_grad_(True)
        V = _uniform(rng, (mat.n, 3), dtype).requires_grad_(True)
        Q1 = _uniform(rng, (mat.m, 4), dtype).requires_grad_(True)
        Q2 = _uniform(rng, (mat.m, 4), dtype).mul_(3).requires_grad_(True)
        dY1, dY2 = _uniform(rng, (mat.m, 3), dtype), _uniform(rng, (mat.m, 3), dtype)
        o1 = autograd.attention(A, Q1, K, V)
        o2 = autograd.attention(A, Q2, K, V)
        (gQ1, gK1, gV1) = torch.autograd.grad(o1, (Q1, K, V), dY1)
        (gQ2, gK2, gV2) = torch.autograd.grad(o2, (Q2, K, V), dY2)
        torch.cuda.synchronize()
        for Q, dY, o, got in ((Q1, dY1, o1, (gQ1, gK1, gV1)), (Q2, dY2, o2, (gQ2, gK2, gV2))):
            want, rQ, rK, rV = _reference(mat, rows, cols, Q, K, V, dY)
            rho, a_out, a_Q, a_K, a_V = _allowances(mat, rows, cols, Q, K, V, dY, dtype)
            what = f"{mat.name} {np.dtype(dtype).name} interleaved"
            _within(o.detach(), want, a_out, what + " out")
            _within(got[0], rQ, a_Q, what + " dQ")
            _within(got[1], rK, a_K, what + " dK")
            _within(got[2], rV, a_V, what + " dV")
        _close(A)


def test_companion_is_built_only_for_a_gradient_of_k_or_v():
    mat = S.duplicates_matrix()
    rng = np.random.default_rng(6)
    rows, cols = _index(mat)
    A = _open(mat, np.float64)
    Q = _uniform(rng, (mat.m, 3), np.float64).requires_grad_(True)
    K = _uniform(rng, (mat.n, 3), np.float64)
    V = _uniform(rng, (mat.n, 2), np.float64)
    dY = _uniform(rng, (mat.m, 2), np.float64)
    autograd.attention(A, Q, K, V).backward(dY)
    torch.cuda.synchronize()
    assert A.info().transpose_built == 0
    want, rQ, _rK, _rV = _reference(mat, rows, cols, Q, K, V, dY)
    _, _, a_Q, _, _ = _allowances(mat, rows, cols, Q, K, V, dY, np.float64)
    _within(Q.grad, rQ, a_Q, "dQ alone")
    # sddmm alone: a gradient for U only needs no companion either, one for V does
    U = _uniform(rng, (mat.m, 3), np.float64).requires_grad_(True)
    G = _uniform(rng, mat.nnz, np.float64)
    autograd.sddmm(A, U, K).backward(G)
    assert A.info().transpose_built == 0
    want_U = torch.zeros_like(U).index_add(0, rows, G[:, None] * K[cols])
    assert torch.allclose(U.grad, want_U, rtol=1e-12, atol=1e-14)
    K.requires_grad_(True)
    autograd.sddmm(A, U, K).backward(G)
    assert A.info().transpose_built == 1
    want_K = torch.zeros_like(K).index_add(0, cols, G[:, None] * U.detach()[rows])
    assert torch.allclose(K.grad, want_K, rtol=1e-12, atol=1e-14)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=("fp64", "fp32"))
def test_a_side_stream_gives_the_same_bits(dtype):
    mat = [m for m in zoo.small_zoo() if m.name == "half-empty"][0]
    rng = np.random.default_rng(7)
    A = _open(mat, dtype)
    Q, K, V = _uniform(rng, (mat.m, 5), dtype), _uniform(rng, (mat.n, 5), dtype), _uniform(rng, (mat.n, 4), dtype)
    dY = _uniform(rng, (mat.m, 4), dtype)

    def run():
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        out = autograd.attention(A, q, k, v)
        out.backward(dY)
        return out.detach(), q.grad, k.grad, v.grad
    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = run()
    side.synchronize()
    torch.cuda.synchronize()
    third = run()  # and back on the default stream
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)
    _close(A)
