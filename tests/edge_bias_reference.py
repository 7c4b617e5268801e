"""The float64 comparison of the edge-bias attention calls (csr5hip_mha_edge_bias, csr5hip_mha_edge_bias_backward): inputs, the
reference and THE ALLOWANCE, restated from tests/test_gpu_mha_bias.py (``_bias_allowances``) and tests/mha_bias_reference.py
(``first_order_rho``) for a bias that is GIVEN in the handle's type instead of being formed as slope * value.  Used by
tests/test_gpu_mha_edge_bias.py; the numpy part is checked without a GPU in tests/test_mha_edge_bias_host.py.

THE ALLOWANCE is tests/test_gpu_attention_autograd.py's (``_allowances``: rho times the expression on absolute values, STAGES rho
for the gradients) with the score-error term sigma derived for THIS score.  The computed score is s^ = fl(qk^ c + b): qk^ the
chain's result, |qk^ - qk| <= sigma_e = gamma(k) sum |q| |k|; b = B[e, h] is an input, exact; c is the scale in the handle's
type, the same number on both sides; the fused multiply-add rounds once, |fl(x) - x| <= u |x| with |x| <= |c qk^| + |b|.  To
first order

    |s^ - s| <= |c| sigma_e + u (|c qk| + |b|) =: sigma'_e,

and sigma' is its maximum over the entries and heads.  (The biased call's term is u (|c qk| + 2 |b|): one u |b| more for the
rounded product slope * value, which does not exist here.)  Everything after the score is csr5hip_mha's, so rho is
``_bias_allowances``' expression with this sigma':

    rho = (2 sigma' + beta + gamma(Lmax)) (1 + 2**-10) (2 in fp64: the reference is computed in fp64 by the same operations),

beta the softmax reference's own relative bound.  dQ and dK carry one more rounding (t = ds c) and the factor |c|: |c| times the
plain allowances, STAGES covering the multiplication as it covers the other stages.  dB = ds has the allowance of ds,
STAGES rho A_s -- and it IS the gradient of B: no reduction follows, so nothing is propagated further.  STAGES and FIRST_ORDER
are tests/test_gpu_attention_autograd.py's; no constant is introduced here."""
import numpy as np

from tests import mha_bias_reference as B


# the cases of the float64 comparison: heads, (k, d), and the seed per matrix
F_HEADS, F_K, F_D = 3, 8, 16
F_SEEDS = {"class-edges": 1700, "random": 1710}


def random_matrix():
    """a small random matrix: 300 x 200, rows of 0 .. 40 entries, columns unsorted, duplicates allowed"""
    from benchmark_spmv_using_csr5_amd import matrices as M
    rng = np.random.default_rng(1720)
    return M.csr_from_row_lengths(rng.integers(0, 41, size=300).astype(np.int64), 200, rng, name="random-300x200")


def transposed(mat):
    """A^T in CSR, every column's entries in A's CSR order (a stable sort by column)"""
    from benchmark_spmv_using_csr5_amd import matrices as M
    rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    order = np.argsort(cols, kind="stable")
    rp = np.zeros(mat.n + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(cols, minlength=mat.n))
    return M.CsrMatrix(mat.n, mat.m, rp, rows[order].astype(np.int32), np.ones(mat.nnz), mat.name + "^T")


def distinct_bias(mat, heads, seed):
    """(nnz, heads) float64 in [-2, 2 + 4 / nnz): column h is ``B.distinct_values(mat, seed + h)`` moved up by h steps of
    4 / (nnz heads), so EVERY (entry, head) holds a value of its own (also in fp32): a bias taken from another entry or from
    another head is an error of order one"""
    cols = [B.distinct_values(mat, seed + h) + h * 4.0 / max(mat.nnz * heads, 1) for h in range(heads)]
    out = np.stack(cols, axis=1) if mat.nnz else np.zeros((0, heads))
    assert len(np.unique(out.astype(np.float32))) == out.size
    return out


def case(mat, heads, k, d, dtype, seed):
    """(B (nnz, heads), c, (Q, K, V, dO)) of `dtype`: a bias in [-2, 2) per entry and head, c = 1 / sqrt(k) in the handle's type,
    operands as tests/test_gpu_mha_bias.py's ``_operands`` draws them (Q in [-2, 2), the others in [-1, 1))"""
    rng = np.random.default_rng([seed, mat.nnz, heads])
    bias = rng.uniform(-2, 2, size=(mat.nnz, heads)).astype(dtype)
    c = float(np.asarray(1 / np.sqrt(k), dtype=dtype))
    u = lambda rows, w: rng.uniform(-1, 1, size=(rows, heads, w)).astype(dtype)  # noqa: E731
    return bias, c, (u(mat.m, k) * dtype(2), u(mat.n, k), u(mat.n, d), u(mat.m, d))


def first_order_rho(mat, c, bias, Q, K, dtype):
    """rho of the module docstring in numpy float64: a function of the inputs and of the reference alone, so the condition
    STAGES * rho <= FIRST_ORDER can be judged without a GPU"""
    from tests import softmax_reference as R
    from tests.exact_reference import unit_roundoff
    u = unit_roundoff(dtype)
    k = Q.shape[2]
    rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    Qd, Kd, bd = (np.asarray(t, dtype=np.float64) for t in (Q, K, bias))
    qk = (Qd[rows] * Kd[cols]).sum(axis=2)
    s = c * qk + bd
    sigma_e = (k * u / (1 - k * u)) * (np.abs(Qd[rows]) * np.abs(Kd[cols])).sum(axis=2)
    sigma = float((abs(c) * sigma_e + u * (np.abs(c * qk) + np.abs(bd))).max())
    beta = 0.0
    for h in range(s.shape[1]):
        ref = R.softmax_reference(mat.row_ptr, s[:, h].astype(dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = max(beta, float(np.nanmax(np.where(ref.expected > 0, ref.bound / ref.expected, 0))))
    Lmax = int(np.diff(mat.row_ptr).max())
    return (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * (1 + 2.0 ** -10) * (2 if np.dtype(dtype) == np.float64 else 1)


def _softmax(torch, m, rows, scores):
    M = torch.full((m,), -float("inf"), dtype=scores.dtype, device=scores.device).scatter_reduce(0, rows, scores.detach(), "amax")
    e = torch.exp(scores - M[rows])
    Z = torch.zeros(m, dtype=scores.dtype, device=scores.device).index_add(0, rows, e)
    return e / Z[rows]


def reference(mat, rows, cols, c, bias, Q, K, V, dO):
    """(O, dQ, dK, dV, dB) by torch autograd in float64, dense-free over (rows, cols); every argument a torch tensor on one device"""
    import torch
    Qr, Kr, Vr, Br = (t.detach().double().clone().requires_grad_(True) for t in (Q, K, V, bias))
    s = c * (Qr[rows] * Kr[cols]).sum(dim=2) + Br
    p = torch.stack([_softmax(torch, mat.m, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    out = torch.zeros((mat.m,) + tuple(Vr.shape[1:]), dtype=torch.float64, device=Qr.device).index_add(0, rows, p[:, :, None] * Vr[cols])
    out.backward(dO.double())
    return out.detach(), Qr.grad, Kr.grad, Vr.grad, Br.grad


def allowances(mat, rows, cols, c, bias, Q, K, V, dO, dtype, stages):
    """(rho, allowances of O, dQ, dK, dV, dB) in float64 torch tensors: the module docstring's, per head; ``stages`` is
    tests/test_gpu_attention_autograd.py's STAGES"""
    import torch
    np_of = lambda t: t.detach().cpu().numpy()  # noqa: E731
    rho = first_order_rho(mat, c, np_of(bias), np_of(Q), np_of(K), dtype)
    dev = Q.device
    Qd, Kd, Vd, dOd, bd = (t.detach().double() for t in (Q, K, V, dO, bias))
    s = c * (Qd[rows] * Kd[cols]).sum(dim=2) + bd
    p = torch.stack([_softmax(torch, mat.m, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    zeros = lambda t: torch.zeros(t.shape, dtype=torch.float64, device=dev)  # noqa: E731
    a_out = torch.zeros((mat.m,) + tuple(Vd.shape[1:]), dtype=torch.float64, device=dev).index_add(0, rows, p[:, :, None] * Vd[cols].abs())
    a_V = zeros(Vd).index_add(0, cols, p[:, :, None] * dOd[rows].abs())
    a_p = (dOd[rows].abs() * Vd[cols].abs()).sum(dim=2)
    a_s = p * (a_p + torch.zeros((mat.m, s.shape[1]), dtype=torch.float64, device=dev).index_add(0, rows, p * a_p)[rows])
    a_Q = abs(c) * zeros(Qd).index_add(0, rows, a_s[:, :, None] * Kd[cols].abs())
    a_K = abs(c) * zeros(Kd).index_add(0, cols, a_s[:, :, None] * Qd[rows].abs())
    return rho, rho * a_out, stages * rho * a_Q, stages * rho * a_K, stages * rho * a_V, stages * rho * a_s
