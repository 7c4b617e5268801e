"""The references of the additive attention calls (csr5hip_gat, csr5hip_gat_backward): THE CHAIN IN NUMPY, BIT FOR BIT, a numpy
float64 reference with the wrong kernels it must reject, the float64 torch-autograd reference and THE ALLOWANCE, restated from
tests/edge_bias_reference.py for a score that is not a dot product.  Used by tests/test_gpu_gat.py and
scripts/host_emulation/run_gat.py; the numpy part is checked without a GPU in tests/test_gat_host.py.

THE SCORE, per stored entry e = (i, j), head h and channel c < k, every operation rounded once:

    u_c = Q[i, h, c] + K[j, h, c];  l_c = u_c > 0 ? u_c : ns u_c;  z = fma(a[h, c], l_c, z) from +0;  s = fma(z, scale, B[e, h]).

THE CHAIN IN NUMPY (``scores``).  With a in {1, 1/2, -1, 2} the product a l_c is exact (a power of two, up to sign), so
fma(a, l_c, z) = fl(a l_c + z) is ONE rounded numpy addition of two numbers of the type; with the scale a power of two z scale is
exact and fma(z, scale, b) = fl(z scale + b) is one rounded addition too; u_c and ns u_c are one numpy operation each.  So numpy
arithmetic in the handle's type restates the score exactly, the sign of a zero included (z starts at +0, and +0 + -0 = +0 in both).
tests/test_gpu_gat.py hands these scores as B' to the edge call with k = 0, which computes fma(+0, scale, B') = B': existing code on
the same scores.

THE ALLOWANCE is tests/test_gpu_attention_autograd.py's (rho times the expression on absolute values, STAGES rho for the
gradients) with the score-error term derived for THIS score.  Let u be the unit roundoff.  u_c^ = fl(q + k) = (q + k)(1 + d1);
fl(q + k) HAS THE SIGN OF q + k (a rounded sum of two numbers of the type is zero only if the exact sum is, and rounding is
monotone), SO THE BRANCH u > 0 OF THE COMPUTED SCORE IS THE EXACT ONE and g, the derivative of the LeakyReLU, is exact on both
sides.  l_c^ = u_c^ or fl(ns u_c^): at most one more rounding, |l_c^ - l_c| <= 2 u |l_c| to first order.  The chain of k fused
multiply-adds adds gamma(k) sum_c |a_c| |l_c| (Higham section 4.2), and the last FMA rounds once as the edge call's does:

    |s^ - s| <= |c| (gamma(k) + 2 u) sum_c |a_c| |l_c| + u (|c z| + |b|) =: sigma'_e,

c the scale in the handle's type (the same number on both sides, as ns is).  sigma' is its maximum over the entries and heads, and
everything after the score is csr5hip_mha's, so rho is edge_bias_reference's expression with this sigma':

    rho = (2 sigma' + beta + gamma(Lmax)) (1 + 2**-10) (2 in fp64: the reference is computed in fp64 by the same operations).

dQ = sum_e t_e w_ec, dK likewise over the column and dAr = sum_e t_e l_ec have the form of the edge call's dQ = sum_e t_e K[j_e, c]
with another second factor: their allowances carry |w| = |a| g resp. |l| in K's / Q's place, A_Q = |c| sum_row A_s |w|,
A_K = |c| sum_col A_s |w|, A_Ar = |c| sum_row A_s |l|, times STAGES rho.  STAGES counts the second factor as one stage within rho of its exact value, as it counts K: w = a g is
one rounded product of an exact g (u <= rho), and l is within 2 u <= rho (rho >= gamma(Lmax) >= 2 u wherever a row has two entries).
dV and dB are the edge call's.  The gradient of a is dAr.sum(0) formed in torch: its allowance is the column sum of dAr's plus
gamma(m) of the sum of |dAr|.  STAGES and FIRST_ORDER are tests/test_gpu_attention_autograd.py's; no constant is introduced here."""
import numpy as np

from tests import mha_bias_reference as B

NAMES = ("O", "dQ", "dK", "dV", "dB", "dAr")
EXACT_A = (1.0, 0.5, -1.0, 2.0)

# the cases of the float64 comparison: heads, (k, d), and the seed per matrix
F_HEADS, F_K, F_D = 3, 8, 16
F_SEEDS = {"class-edges": 2700, "random": 2710}
F_SLOPE = 0.2


def rows_cols(mat):
    return B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)


def exact_a(heads, k, dtype):
    """(heads, k) of the values for which the chain is restated exactly, a different cycle per head"""
    return np.array([[EXACT_A[(h + 2 * c) % 4] for c in range(k)] for h in range(heads)], dtype=dtype).reshape(heads, k)


def scores(mat, Q, K, a, ns, scale, bias, dtype):
    """(nnz, H) of `dtype`: the definition's scores, bit for bit (the module docstring).  a: (H, k) with entries of EXACT_A, or
    None; scale: a power of two; bias: (nnz, H) or None"""
    rows, cols = rows_cols(mat)
    m, e = np.frexp(abs(scale))
    assert m == 0.5, "the scale must be a power of two"
    assert a is None or np.isin(np.asarray(a, dtype=np.float64), EXACT_A).all()
    Q, K = np.asarray(Q, dtype=dtype), np.asarray(K, dtype=dtype)
    heads, k = Q.shape[1], Q.shape[2]
    nst, ct = dtype(ns), dtype(scale)
    with np.errstate(invalid="ignore", over="ignore"):
        u = Q[rows] + K[cols]                                  # one rounded addition
        l = np.where(u > 0, u, nst * u)                        # one rounded multiplication
        z = np.zeros((mat.nnz, heads), dtype=dtype)
        for c in range(k):
            al = l[:, :, c] if a is None else np.asarray(a, dtype=dtype)[None, :, c] * l[:, :, c]  # exact
            z = al + z                                         # fma(a, l, z): one rounding
        b = np.zeros((mat.nnz, heads), dtype=dtype) if bias is None else np.asarray(bias, dtype=dtype)
        s = z * ct + b                                         # z c exact: fma(z, c, b), one rounding
    assert s.dtype == np.dtype(dtype)
    return s


def _scatter(idx, n, terms):
    out = np.zeros((n,) + terms.shape[1:])
    np.add.at(out, idx, terms)
    return out


def numpy_reference(mat, a, ns, scale, bias, Q, K, V, dO, wrong=None):
    """((O, dQ, dK, dV, dB, dAr), the same expressions on absolute values, the largest score magnitude) in numpy float64.  a (H, k)
    or None, bias (nnz, H) or None.  wrong: None, or a wrong kernel to model -- "g-from-la": g taken from the sign of l a instead of
    u's (dQ and dK); "a-of-head-0": the attention vector of head 0 used for every head (everything)."""
    Q, K, V, dO = (np.asarray(t, dtype=np.float64) for t in (Q, K, V, dO))
    rows, cols = rows_cols(mat)
    H, k = Q.shape[1], Q.shape[2]
    aa = np.ones((H, k)) if a is None else np.asarray(a, dtype=np.float64)
    if wrong == "a-of-head-0":
        aa = np.repeat(aa[:1], H, axis=0)
    bb = np.zeros((mat.nnz, H)) if bias is None else np.asarray(bias, dtype=np.float64)
    u = Q[rows] + K[cols]
    l = np.where(u > 0, u, ns * u)
    g = np.where((l * aa[None] if wrong == "g-from-la" else u) > 0, 1.0, ns)
    w = aa[None] * g
    z = (aa[None] * l).sum(2)
    s = scale * z + bb
    mx = np.full((mat.m, H), -np.inf)
    np.maximum.at(mx, rows, s)
    e = np.exp(s - mx[rows])
    p = e / _scatter(rows, mat.m, e)[rows]
    dp, adp = (dO[rows] * V[cols]).sum(2), (np.abs(dO[rows]) * np.abs(V[cols])).sum(2)
    ds = p * (dp - _scatter(rows, mat.m, p * dp)[rows])
    ads = p * (adp + _scatter(rows, mat.m, p * adp)[rows])
    t, at = scale * ds, abs(scale) * ads
    got = (_scatter(rows, mat.m, p[:, :, None] * V[cols]), _scatter(rows, mat.m, t[:, :, None] * w),
           _scatter(cols, mat.n, t[:, :, None] * w), _scatter(cols, mat.n, p[:, :, None] * dO[rows]), ds,
           _scatter(rows, mat.m, t[:, :, None] * l))
    mag = (_scatter(rows, mat.m, p[:, :, None] * np.abs(V[cols])), _scatter(rows, mat.m, at[:, :, None] * np.abs(w)),
           _scatter(cols, mat.n, at[:, :, None] * np.abs(w)), _scatter(cols, mat.n, p[:, :, None] * np.abs(dO[rows])), ads,
           _scatter(rows, mat.m, at[:, :, None] * np.abs(l)))
    smag = float((abs(scale) * (np.abs(aa[None]) * np.abs(l)).sum(2) + np.abs(bb)).max()) if mat.nnz else 0.0
    return got, mag, smag


def within(g, r, a, smag, u):
    """elementwise: |g - r| <= 1e3 unit roundoffs of the expression on absolute values, times one plus the largest score magnitude
    (NaN is outside): the host emulation's check of the indexing, scripts/host_emulation/emulation.py's"""
    return np.abs(g - r) <= 1e3 * u * (1 + smag) * np.maximum(a, 1e-30) + 1e-300


def random_matrix():
    from tests import edge_bias_reference as EB
    return EB.random_matrix()


def case(mat, heads, k, d, dtype, seed):
    """(a (heads, k), ns, bias (nnz, heads), c, (Q, K, V, dO)) of `dtype`: a in [-1, 1), ns = F_SLOPE and c = 1 / sqrt(k) in the
    handle's type (as floats), a bias in [-2, 2), Q in [-2, 2), the others in [-1, 1)"""
    rng = np.random.default_rng([seed, mat.nnz, heads])
    bias = rng.uniform(-2, 2, size=(mat.nnz, heads)).astype(dtype)
    a = rng.uniform(-1, 1, size=(heads, k)).astype(dtype)
    c = float(np.asarray(1 / np.sqrt(k), dtype=dtype))
    ns = float(np.asarray(F_SLOPE, dtype=dtype))
    u = lambda rows, w: rng.uniform(-1, 1, size=(rows, heads, w)).astype(dtype)  # noqa: E731
    return a, ns, bias, c, (u(mat.m, k) * dtype(2), u(mat.n, k), u(mat.n, d), u(mat.m, d))


def first_order_rho(mat, c, a, ns, bias, Q, K, dtype):
    """rho of the module docstring in numpy float64: a function of the inputs and of the reference alone, so the condition
    STAGES * rho <= FIRST_ORDER can be judged without a GPU"""
    from tests import softmax_reference as R
    from tests.exact_reference import unit_roundoff
    u = unit_roundoff(dtype)
    k = Q.shape[2]
    rows, cols = rows_cols(mat)
    Qd, Kd, bd, ad = (np.asarray(t, dtype=np.float64) for t in (Q, K, bias, a))
    uu = Qd[rows] + Kd[cols]
    l = np.where(uu > 0, uu, ns * uu)
    z = (ad[None] * l).sum(axis=2)
    s = c * z + bd
    al = (np.abs(ad[None]) * np.abs(l)).sum(axis=2)
    sigma = float((abs(c) * (k * u / (1 - k * u) + 2 * u) * al + u * (np.abs(c * z) + np.abs(bd))).max())
    beta = 0.0
    for h in range(s.shape[1]):
        ref = R.softmax_reference(mat.row_ptr, s[:, h].astype(dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = max(beta, float(np.nanmax(np.where(ref.expected > 0, ref.bound / ref.expected, 0))))
    Lmax = int(np.diff(mat.row_ptr).max())
    return (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * (1 + 2.0 ** -10) * (2 if np.dtype(dtype) == np.float64 else 1)


def _softmax(torch, m, rows, s):
    M = torch.full((m,), -float("inf"), dtype=s.dtype, device=s.device).scatter_reduce(0, rows, s.detach(), "amax")
    e = torch.exp(s - M[rows])
    Z = torch.zeros(m, dtype=s.dtype, device=s.device).index_add(0, rows, e)
    return e / Z[rows]


def _score(torch, rows, cols, c, a, ns, bias, Q, K):
    l = torch.nn.functional.leaky_relu(Q[rows] + K[cols], ns)
    z = (l * a[None]).sum(dim=2) if a is not None else l.sum(dim=2)
    return (c * z + bias if bias is not None else c * z), l


def reference(mat, rows, cols, c, a, ns, bias, Q, K, V, dO):
    """(O, dQ, dK, dV, dB, dAr, da) by torch autograd in float64, dense-free over (rows, cols); every argument a torch tensor on
    one device, a and bias may be None (dB, da then None; dAr is formed from the reference's own ds: c ds l summed over the row)"""
    import torch
    Qr, Kr, Vr = (t.detach().double().clone().requires_grad_(True) for t in (Q, K, V))
    ar = a.detach().double().clone().requires_grad_(True) if a is not None else None
    Br = bias.detach().double().clone().requires_grad_(True) if bias is not None else None
    s, l = _score(torch, rows, cols, c, ar, ns, Br, Qr, Kr)
    s.retain_grad()
    p = torch.stack([_softmax(torch, mat.m, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    out = torch.zeros((mat.m,) + tuple(Vr.shape[1:]), dtype=torch.float64, device=Qr.device).index_add(0, rows, p[:, :, None] * Vr[cols])
    out.backward(dO.double())
    ds = s.grad
    dAr = torch.zeros_like(Qr).index_add(0, rows, (c * ds)[:, :, None] * l.detach())
    return (out.detach(), Qr.grad, Kr.grad, Vr.grad, ds if Br is None else Br.grad, dAr, ar.grad if ar is not None else None)


def allowances(mat, rows, cols, c, a, ns, bias, Q, K, V, dO, dtype, stages):
    """(rho, allowances of O, dQ, dK, dV, dB, dAr, da) in float64 torch tensors: the module docstring's, per head; ``stages`` is
    tests/test_gpu_attention_autograd.py's STAGES"""
    import torch
    from tests.exact_reference import unit_roundoff
    np_of = lambda t: t.detach().cpu().numpy()  # noqa: E731
    ones = torch.ones((Q.shape[1], Q.shape[2]), dtype=torch.float64, device=Q.device)
    ad = a.detach().double() if a is not None else ones
    zb = torch.zeros((mat.nnz, Q.shape[1]), dtype=torch.float64, device=Q.device)
    bd = bias.detach().double() if bias is not None else zb
    rho = first_order_rho(mat, c, np_of(ad), ns, np_of(bd), np_of(Q), np_of(K), dtype)
    dev = Q.device
    Qd, Kd, Vd, dOd = (t.detach().double() for t in (Q, K, V, dO))
    s, l = _score(torch, rows, cols, c, ad, ns, bd, Qd, Kd)
    uu = Qd[rows] + Kd[cols]
    w = ad[None].abs() * torch.where(uu > 0, torch.ones_like(uu), torch.full_like(uu, abs(ns)))
    p = torch.stack([_softmax(torch, mat.m, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    zeros = lambda t: torch.zeros(t.shape, dtype=torch.float64, device=dev)  # noqa: E731
    a_out = torch.zeros((mat.m,) + tuple(Vd.shape[1:]), dtype=torch.float64, device=dev).index_add(0, rows, p[:, :, None] * Vd[cols].abs())
    a_V = zeros(Vd).index_add(0, cols, p[:, :, None] * dOd[rows].abs())
    a_p = (dOd[rows].abs() * Vd[cols].abs()).sum(dim=2)
    a_s = p * (a_p + torch.zeros((mat.m, s.shape[1]), dtype=torch.float64, device=dev).index_add(0, rows, p * a_p)[rows])
    a_Q = abs(c) * zeros(Qd).index_add(0, rows, a_s[:, :, None] * w)
    a_K = abs(c) * zeros(Kd).index_add(0, cols, a_s[:, :, None] * w)
    a_Ar = abs(c) * zeros(Qd).index_add(0, rows, a_s[:, :, None] * l.abs())
    u = unit_roundoff(dtype)
    gm = mat.m * u / (1 - mat.m * u)
    a_a = stages * rho * a_Ar.sum(0) + gm * (1 + stages * rho) * a_Ar.sum(0)  # (|dAr| <= A_Ar: the torch column sum's own error)
    return rho, rho * a_out, stages * rho * a_Q, stages * rho * a_K, stages * rho * a_V, stages * rho * a_s, stages * rho * a_Ar, a_a
