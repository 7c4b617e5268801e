"""Exact expectations for the biased attention calls (csr5hip_mha_biased, csr5hip_mha_biased_backward) from the PLAIN calls on
AUGMENTED OPERANDS (numpy only, no GPU).  Used by tests/test_gpu_mha_bias.py and checked in tests/test_mha_bias_host.py.

With a bias of rank one, a_e = u[i_e] * v[j_e], integer-valued u and v in [-4, 4] (so the product is exact), scale 1 and a slope
per head from {1, 2, 0.5, -1} (so slope_h * a_e is exact too), the biased score of the definition is

    s = fma(qk, 1, slope_h u_i v_j) = round(qk + slope_h u_i v_j)

and the plain chain over Q widened by the column u and K widened by the column slope_h v continues qk, its first k steps
unchanged, with ONE more fused multiply-add, fma(u_i, slope_h v_j, qk) = round(u_i slope_h v_j + qk): the same real number
rounded once, the same bits.  Everything after the score is shared, so O and dV of the biased call have the bits of the plain
call on the widened operands; ds has them too, hence dQ = sum ds K and dK = sum ds Q (t = ds * 1) equal the first k columns of the
widened gradients WHERE THE SUMMATION ORDER IS THE SAME: the accumulation is per output column, but beyond 16 entries its slot
count is a function of the smallest power of two >= the width (csr5_attention.hip, acc_c), so k and k + 1 must round up to the
same power of two (k = 5, 6 or 7; 9 .. 15; ...)."""
import numpy as np

SLOPES = (1.0, 2.0, 0.5, -1.0)


def rows_of(mat):
    return np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))


def rank_one(mat, seed):
    """(u (m,), v (n,), a (nnz,)) in float64: integers in [-4, 4] and a_e = u[i_e] * v[j_e], exact in fp32 and fp64"""
    rng = np.random.default_rng([seed, mat.m, mat.n])
    u = rng.integers(-4, 5, size=mat.m).astype(np.float64)
    v = rng.integers(-4, 5, size=mat.n).astype(np.float64)
    return u, v, u[rows_of(mat)] * v[mat.col[:mat.nnz].astype(np.int64)]


def augment(Q, K, u, v, slopes=None):
    """Q (m, H, k), K (n, H, k) -> Q|u (m, H, k + 1), K|slope_h v (n, H, k + 1), contiguous, of Q's dtype"""
    m, H, k = Q.shape
    s = np.ones(H) if slopes is None else np.asarray(slopes, dtype=np.float64)
    assert all(x in SLOPES for x in s), "only slopes that keep the products exact"
    Qw = np.empty((m, H, k + 1), dtype=Q.dtype)
    Kw = np.empty((K.shape[0], H, k + 1), dtype=K.dtype)
    Qw[:, :, :k], Kw[:, :, :k] = Q, K
    Qw[:, :, k] = u[:, None]
    Kw[:, :, k] = v[:, None] * s[None, :]
    return Qw, Kw
