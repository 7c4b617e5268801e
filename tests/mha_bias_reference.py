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


def augment(Q, K, u, v, slopes=None, pad=0):
    """Q (m, H, k), K (n, H, k) -> Q|u|0 (m, H, k + 1 + pad), K|slope_h v|0 (n, H, k + 1 + pad), contiguous, of Q's dtype: the bias
    column, then ``pad`` columns of +0 in BOTH operands (a width such as 12 + 1 + 3 = 16, at which the widened call takes the
    16-byte loads the biased call takes at 12).

    WHY THE BITS SURVIVE THE PADDING.  After the bias column the chain holds x = round(qk + b), the biased score.  Every padding
    step is fma(+0, +0, x): the product is exactly +0 and x + (+0) is x, for every finite x, every infinity and NaN.  The one
    value that a sum with +0 changes is -0, and x is never -0 on either side: the chain starts from +0 and a sum onto +0 can give
    -0 only from two negative zeros (round to nearest: (+0) + (-0) = +0, and an exact cancellation of non-zero terms gives +0), so
    no partial sum of the plain chain is -0; on the biased side qk is such a partial sum, qk * c with c > 0 is +0 or non-zero,
    and fma(qk, c, b) with b = -0 gives (+0) + (-0) = +0, with b = -(qk c) the cancellation's +0.  So the sign of zero cannot
    differ either: round(qk + b) has the same bits on both sides, before and after the padding."""
    m, H, k = Q.shape
    s = np.ones(H) if slopes is None else np.asarray(slopes, dtype=np.float64)
    assert all(x in SLOPES for x in s), "only slopes that keep the products exact"
    assert pad >= 0
    Qw = np.zeros((m, H, k + 1 + pad), dtype=Q.dtype)
    Kw = np.zeros((K.shape[0], H, k + 1 + pad), dtype=K.dtype)
    Qw[:, :, :k], Kw[:, :, :k] = Q, K
    Qw[:, :, k] = u[:, None]
    Kw[:, :, k] = v[:, None] * s[None, :]
    return Qw, Kw


def scaled_identity(c):
    """the scale c as a float, after asserting that it is a power of two 2**e with -8 <= e <= 0: the condition of the identity

        mhaBiased(scale = c, bias b) on Q, K   ==   mha on c Q | u | 0 and K | slope v | 0,   bit for bit,

    which tests/test_gpu_mha_bias_edges.py (A) uses.  A multiplication by 2**e changes the exponent alone, so it commutes with
    every rounding whose result is not subnormal:
      * the plain chain on c Q: every step is fma(c q, k, c acc) = c fma(q, k, acc), so after k steps it holds exactly c qk, qk
        the chain on Q; the bias step gives round(c qk + b), which is fma(qk, c, b), the biased score;
      * dK: the biased call sums t Q with t = round(ds c) = ds c (exact), the widened call ds (c Q): the same products;
      * dQ: the biased call sums (ds c) K, every step c times the step of the widened call's sum of ds K: c times its result.
    All of it holds while no operand, product coefficient or partial result is subnormal (there c x may lose bits that x has):
    the callers assert that on their data (``no_subnormal``)."""
    c = float(c)
    mant, exp = np.frexp(c)
    assert mant == 0.5 and -8 <= exp - 1 <= 0, f"{c} is no power of two in [2**-8, 1]"
    return c


def no_subnormal(a, factor=1.0, margin=2.0 ** 24) -> bool:
    """every element of a is zero, not finite, or at least ``margin`` smallest normals of its type in magnitude after the
    multiplication by ``factor`` (margin 1: the product is a normal number, so the multiplication is exact)"""
    a = np.asarray(a)
    mag = np.abs(a[np.isfinite(a) & (a != 0)].astype(np.float64)) * abs(factor)
    return bool((mag >= float(np.finfo(a.dtype).tiny) * margin).all())


def score_spread(mat, c, qk, b):
    """the largest (max - min of a row's scores c qk + b) + ln(row length) over the rows and heads, in float64: every softmax
    weight p of the call is at least exp(-this), since w >= exp(min - max) and Z <= L"""
    s = c * np.asarray(qk, dtype=np.float64) + b
    rows, lens = rows_of(mat), np.diff(mat.row_ptr)
    mx, mn = np.full((mat.m, s.shape[1]), -np.inf), np.full((mat.m, s.shape[1]), np.inf)
    np.maximum.at(mx, rows, s)
    np.minimum.at(mn, rows, s)
    some = lens > 0
    return float(((mx - mn)[some] + np.log(lens[some])[:, None]).max())


def distinct_values(mat, seed):
    """(nnz,) float64: a permutation of nnz equidistant values in [-2, 2), as scripts/host_emulation/run_mha_bias.py uses -- every
    entry's value is distinct (also in fp32: the step 4 / nnz is far above 2**-22), so a value taken from another entry's
    position is an error of order one, not of one unit in the last place"""
    val = np.random.default_rng([seed, mat.nnz]).permutation(mat.nnz) / max(mat.nnz, 1) * 4 - 2
    assert len(np.unique(val.astype(np.float32))) == mat.nnz
    return val


def vec_forward(heads, k, itemsize, ldq, ldk, q_addr=0, k_addr=0) -> bool:
    """attention_vec of csr5_attention_kern.h, transcribed: does the forward take 16-byte loads?"""
    return (k >= 32 // itemsize and q_addr % 16 == 0 and k_addr % 16 == 0 and (ldq * itemsize) % 16 == 0 and (ldk * itemsize) % 16 == 0
            and (heads == 1 or (k * itemsize) % 16 == 0))


def vec_backward(heads, k, d, itemsize, lds, addrs=(0, 0, 0, 0)) -> bool:
    """attention_bwd_vec of csr5_attention_bwd_kern.h, transcribed; lds / addrs: the leading dimensions / addresses of Q, K, V, dO"""
    vec = heads == 1 or ((k * itemsize) % 16 == 0 and (d * itemsize) % 16 == 0)
    return vec and all(a % 16 == 0 and (ld * itemsize) % 16 == 0 for a, ld in zip(addrs, lds))


# ---- the score of the definition and wrong scores, in numpy (one rounding per operation; fp32 through float64) -------------------
def _fma(x, y, z, dtype):
    """round(x y + z) in float32, from float64: the product of two floats is exact there; its sum with a float is rounded to 53
    bits and then to 24.  The two roundings equal one unless the float64 sum is INEXACT and lands exactly half-way between two
    floats; the error of the sum is computed (two-sum) and that case is asserted not to occur, so every value returned is the
    correctly rounded one.  (fp64 would need exact rationals: tests/test_mha_bias_host.py does that on a cut.)"""
    assert np.dtype(dtype) == np.float32
    p, z = x.astype(np.float64) * y.astype(np.float64), z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        wide = p + z
        t = wide - p
        err = (p - (wide - t)) + (z - t)
        out = wide.astype(np.float32)
        tie = np.abs(wide - out.astype(np.float64)) * 2 == np.spacing(np.abs(out)).astype(np.float64)
    assert not (tie & (err != 0) & np.isfinite(wide)).any(), "an inexact float64 sum on a float32 tie: double rounding"
    return out


def chain(Qe, Ke):
    """the chain of the definition over the last axis of float32 operands: acc = fma(q_c, k_c, acc) from +0"""
    acc = np.zeros(Qe.shape[:-1], dtype=np.float32)
    for c in range(Qe.shape[-1]):
        acc = _fma(Qe[..., c], Ke[..., c], acc, np.float32)
    return acc


SCORES = ("definition", "scale after the sum", "slope ignored", "first head's slope", "neighbour's value")


def scores(kind, qk, c, a, slopes, row_ptr):
    """(nnz, H) float32: the biased score of the definition, s = fma(qk, c, slopes[h] * a), or one of the wrong scores a kernel
    could compute; qk (nnz, H) the chain's result, a (nnz,) the values.  The neighbour is the next entry of the row (the first
    one for the row's last entry), so a row of one entry has none."""
    f = np.float32
    qk, a, c = qk.astype(f), np.asarray(a).astype(f), f(c)
    sl = np.ones(qk.shape[1], dtype=f) if slopes is None else np.asarray(slopes).astype(f)
    if kind == "neighbour's value":
        lens = np.diff(row_ptr)
        first = np.repeat(row_ptr[:-1], lens)
        rank = np.arange(a.size) - first
        a = a[first + (rank + 1) % np.repeat(lens, lens)]
    if kind == "first head's slope":
        sl = np.full_like(sl, sl[0])
    b = (sl[None, :] * a[:, None]).astype(f)          # one rounded multiplication
    if kind == "slope ignored":
        b = np.broadcast_to(a[:, None], qk.shape).astype(f)
    cc = np.broadcast_to(c, qk.shape).astype(f)
    if kind == "scale after the sum":
        return ((qk + b).astype(f) * cc).astype(f)
    return _fma(qk, cc, b, f)


# ---- the operands of tests/test_gpu_mha_bias_edges.py (A), in numpy, so that the host tests judge the same numbers ----------------
A_HEADS, A_K, A_PAD, A_D = 3, 12, 3, 8
A_SLOPES = (2.0, 0.5, -1.0)
A_SCALES = (1.0, 0.25)


def operands_a(mat, dtype, seed=1100):
    """(Q (m, 3, 12) in [-2, 2), K (n, 3, 12), V (n, 3, 8), dO (m, 3, 8) in [-1, 1)), contiguous, of `dtype`"""
    rng = np.random.default_rng([seed, mat.m, mat.n, 64 if np.dtype(dtype) == np.float64 else 32])
    u = lambda rows, w: rng.uniform(-1, 1, size=(rows, A_HEADS, w)).astype(dtype)  # noqa: E731
    return u(mat.m, A_K) * dtype(2), u(mat.n, A_K), u(mat.n, A_D), u(mat.m, A_D)


# ---- the cases of the float64 comparison at the class edges (F), in numpy ---------------------------------------------------------
F_HEADS = 2
F_KD = ((8, 16), (3, 5))


def case_f(mat, k, d, dtype, seed):
    """(val (nnz,), slopes (2,), c, (Q, K, V, dO)) of `dtype`: values in [-2, 2), slopes in [-1.5, 1.5) and c = 1 / sqrt(k) in the
    handle's type as tests/test_gpu_mha_bias.py's ``_case_f`` draws them, operands as its ``_operands`` (Q in [-2, 2), the
    others in [-1, 1))"""
    rng = np.random.default_rng([seed, mat.nnz])
    val = rng.uniform(-2, 2, size=mat.nnz).astype(dtype)
    slopes = rng.uniform(-1.5, 1.5, size=F_HEADS).astype(dtype)
    c = float(np.asarray(1 / np.sqrt(k), dtype=dtype))
    rng = np.random.default_rng([seed + 1, F_HEADS, k, d, 64 if np.dtype(dtype) == np.float64 else 32])
    u = lambda rows, w: rng.uniform(-1, 1, size=(rows, F_HEADS, w)).astype(dtype)  # noqa: E731
    return val, slopes, c, (u(mat.m, k) * dtype(2), u(mat.n, k), u(mat.n, d), u(mat.m, d))


def first_order_rho(mat, c, val, slopes, Q, K, dtype):
    """rho of tests/test_gpu_mha_bias.py's ``_bias_allowances``, the same expression in numpy float64: a function of the inputs
    and of the reference alone, so the condition STAGES * rho <= FIRST_ORDER can be judged without a GPU"""
    from tests import softmax_reference as R
    from tests.exact_reference import unit_roundoff
    u = unit_roundoff(dtype)
    k = Q.shape[2]
    rows, cols = rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    Qd, Kd, ad, sd = (np.asarray(t, dtype=np.float64) for t in (Q, K, val, slopes))
    qk = (Qd[rows] * Kd[cols]).sum(axis=2)
    b = sd[None, :] * ad[:, None]
    s = c * qk + b
    sigma_e = (k * u / (1 - k * u)) * (np.abs(Qd[rows]) * np.abs(Kd[cols])).sum(axis=2)
    sigma = float((abs(c) * sigma_e + u * (np.abs(c * qk) + 2 * np.abs(b))).max())
    beta = 0.0
    for h in range(s.shape[1]):
        ref = R.softmax_reference(mat.row_ptr, s[:, h].astype(dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = max(beta, float(np.nanmax(np.where(ref.expected > 0, ref.bound / ref.expected, 0))))
    Lmax = int(np.diff(mat.row_ptr).max())
    return (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * (1 + 2.0 ** -10) * (2 if np.dtype(dtype) == np.float64 else 1)


def tile_structure(fmt, nnz):
    """(fast-track tiles, entries of the CSR tail) of a converted pattern (the oracle's Csr5Format) as the attention kernels see
    it (att_storage of csr5_attention_dev.h): the first p - 1 tiles are in tile order unless tile_ptr[t] == tile_ptr[t + 1] (no
    row starts inside the tile: it stays in CSR order), everything beyond them is the tail, in CSR order"""
    tiles = max(fmt.p - 1, 0)
    tp = fmt.tile_ptr.astype(np.int64)
    return int((tp[:tiles] == tp[1:tiles + 1]).sum()), int(nnz - tiles * fmt.omega * fmt.sigma)
