"""What tests/test_gpu_mha_lowp_backward.py and tests/test_mha_lowp_backward_host.py share (numpy only, no GPU): the inputs of the
float64 comparison of csr5hip_mha_lowp_backward and the bias of its word identities.

``f64_case`` is tests/lowp_reference.f64_case -- B, Q, K and V uniform in [-1, 1), rounded once to the operand type, the scale
float32(1 / sqrt(k)) -- with dO drawn likewise from the same generator after them, so the four forward operands are that
function's words.  ``rho`` is tests/edge_bias_reference.first_order_rho on the widened operands in float32: what the kernel
computes before it stores."""
import numpy as np

from tests import edge_bias_reference as EB
from tests import lowp_reference as L

F_SEED = 2400


def f64_case(mat, kind, heads, k, d, seed=F_SEED):
    """((B, Q, K, V, dO) as uint16 words, scale)"""
    rng = np.random.default_rng([seed, mat.nnz, len(kind)])
    shapes = ((mat.nnz, heads), (mat.m, heads, k), (mat.n, heads, k), (mat.n, heads, d), (mat.m, heads, d))
    words = tuple(L.to_words(rng.uniform(-1, 1, size=s).astype(np.float32), kind) for s in shapes)
    return words, float(np.float32(1 / np.sqrt(k)))


def rho(mat, kind, heads, k, d, seed=F_SEED):
    words, scale = f64_case(mat, kind, heads, k, d, seed)
    B, Q, K = (L.widen(w, kind) for w in words[:3])
    return EB.first_order_rho(mat, scale, B, Q, K, np.float32)


def masked_bias(mat, words, kind):
    """``words`` (nnz, heads) with -Inf in head 0 only: in every seventh entry, and in ALL entries of the first row of two or more
    entries (a fully masked row: NaN in that row and head, and in the columns it touches).  Returns (words, that row)."""
    out = words.copy()
    ninf = L.to_words(np.array([-np.inf], dtype=np.float32), kind)[0]
    if mat.nnz == 0:
        return out, -1
    out[::7, 0] = ninf
    lens = np.diff(mat.row_ptr)
    row = int(np.flatnonzero(lens >= 2)[0]) if (lens >= 2).any() else int(np.flatnonzero(lens >= 1)[0])
    out[int(mat.row_ptr[row]):int(mat.row_ptr[row + 1]), 0] = ninf
    return out, row
