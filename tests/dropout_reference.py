"""The references of the dropped attention calls (csr5hip_dropout_mha, csr5hip_dropout_gat, their backwards, csr5hip_dropout_mask):
THE MASK IN NUMPY, BIT FOR BIT, a numpy float64 reference of the dropped attention forward and backward with the wrong kernels it
must reject, and THE ALLOWANCE.  Used by tests/test_gpu_attention_dropout.py; the numpy part is checked without a GPU in
tests/test_attention_dropout_host.py.

THE MASK (include/csr5hip_dropout.h).  Philox4x32-10; for the entry of CSR rank e in the PARENT's pattern and the absolute head
g = head0 + h: counter = (e, g >> 2, offset low, offset high), key = (seed low, seed high), dropped = word[g & 3] < thr with
thr = min(llrint(p 2^32), 2^32 - 1).  ``philox4x32_10`` is the 20-line restatement (uint64 products, 10 rounds, the key bumped
after each round); ``mask`` returns 1 for kept.

THE FUNCTION.  With p_e the softmax over ALL stored entries of the row, g_e = keep_e cd, cd = (VT)(1 / (1 - p)):

    O_i = sum_row p_e g_e V_j;  dp_e = g_e (dO_i . V_j);  D_i = sum_row p_e dp_e;  ds_e = p_e (dp_e - D_i);
    dQ_i = c sum_row ds_e K_j;  dK_j = c sum_col ds_e Q_i;  dV_j = sum_col p_e g_e dO_i;  dB_e = ds_e.

THE ALLOWANCE is tests/edge_bias_reference.py's, derived the same way.  cd is a number of the handle's type, the same on both
sides; g_e in {+0, cd} is exact.  Against the undropped call the kernels make TWO MORE ROUNDINGS on any path from the inputs to an
output: forward, rinv cd (one; the weight keep ? w : +0 is exact); backward, g_e (chain) in dp and, for dV, p_e g_e.  Each is a
relative perturbation of at most u of a factor of the term, so rho' = rho + 2 u (1 + 2**-10) (doubled in fp64 as rho is: the
reference makes the same operations in fp64), rho being ``edge_bias_reference.first_order_rho`` on the scores -- which dropout does
not touch: M, w, Z are the undropped call's.  The expressions on absolute values are edge_bias_reference's with p_e g_e in p_e's
place wherever p_e multiplies V or dO, and with A_p = g_e |dO| . |V|: SCALED BY cd on the kept entries and zero on the dropped
ones.  A sum over the kept entries of a row is a sub-sum of the row's: gamma(Lmax) covers it.  A bias of -Inf gives the weight
exactly +0 on both sides: such entries are left out of sigma' and of the softmax reference's bound (the softmax over a row with
-Inf entries IS the softmax over its finite ones); a row masked entirely in a head is NaN in that head on both sides, which
``compare`` demands position by position.  STAGES and FIRST_ORDER are tests/test_gpu_attention_autograd.py's."""
import numpy as np

from tests import mha_bias_reference as B

NAMES = ("O", "dQ", "dK", "dV", "dB")
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """the four output words (uint32 arrays) of the blocks of ``counter`` (four arrays or ints) under ``key`` (two)"""
    lo = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & lo for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & lo for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo]
        k = [(k[0] + np.uint64(W0)) & lo, (k[1] + np.uint64(W1)) & lo]
    return [x.astype(np.uint32) for x in c]


def threshold(p: float) -> int:
    """thr of the definition: min(llrint(p 2^32), 2^32 - 1); rint is llrint's rounding (to nearest, ties to even)"""
    assert 0.0 <= p < 1.0
    return min(int(np.rint(np.float64(p) * 4294967296.0)), 2 ** 32 - 1)


def cd_of(p: float, dtype):
    """cd = (VT)(1 / (1 - p)), formed in double and converted once"""
    return np.dtype(dtype).type(np.float64(1.0) / (np.float64(1.0) - np.float64(p)))


def mask(nnz: int, heads: int, p: float, seed: int, offset: int, head0: int = 0) -> np.ndarray:
    """(nnz, heads) uint8: 1 where head head0 + h of the entry of CSR rank e is KEPT"""
    out = np.zeros((nnz, heads), dtype=np.uint8)
    e = np.arange(nnz, dtype=np.uint64)
    thr = np.uint32(threshold(p))
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for group in sorted({(head0 + h) >> 2 for h in range(heads)}):
        words = philox4x32_10((e, np.full(nnz, group, dtype=np.uint64), np.full(nnz, offset & 0xFFFFFFFF, dtype=np.uint64),
                               np.full(nnz, offset >> 32, dtype=np.uint64)), key)
        for h in range(heads):
            if (head0 + h) >> 2 == group:
                out[:, h] = words[(head0 + h) & 3] >= thr
    return out


def rows_cols(mat):
    return B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)


def _scatter(idx, n, terms):
    out = np.zeros((n,) + terms.shape[1:])
    np.add.at(out, idx, terms)
    return out


def companion_positions(mat):
    """pos (nnz,): the position in A^T's CSR order of the entry of CSR rank e of A (the inverse of the companion's source map)"""
    _, cols = rows_cols(mat)
    order = np.argsort(cols, kind="stable")  # the source map: position in A^T -> rank in A
    pos = np.empty(mat.nnz, dtype=np.int64)
    pos[order] = np.arange(mat.nnz)
    return pos


def numpy_reference(mat, c, bias, Q, K, V, dO, keep, cd, wrong=None, gat=None):
    """((O, dQ, dK, dV, dB), the same expressions on absolute values) in numpy float64: the module docstring's function.  bias
    (nnz, H) or None; keep (nnz, H) of 0 / 1 by the PARENT's CSR rank; cd a number.  wrong: None, or a wrong kernel to model --
    "z-over-kept": Z summed over the kept entries only (a softmax over the survivors, everything); "mask-by-companion-position":
    the column side indexes the mask by the entry's position in A^T's CSR order instead of its rank in A's (dK and dV).
    gat: None, or (a, ns) -- a (H, k) or None, ns the negative slope -- for the ADDITIVE call: the score is c sum_c a_c l_c + bias
    with u = Q_i + K_j, l = LeakyReLU(u); dQ and dK take w = a g (g = u > 0 ? 1 : ns) in K's and Q's place, and a sixth output
    dAr_i = c sum_row ds_e l_e follows."""
    Q, K, V, dO = (np.asarray(t, dtype=np.float64) for t in (Q, K, V, dO))
    rows, cols = rows_cols(mat)
    H = Q.shape[1]
    bb = np.zeros((mat.nnz, H)) if bias is None else np.asarray(bias, dtype=np.float64)
    g = np.asarray(keep, dtype=np.float64) * float(cd)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if gat is None:
            kq, qk_ = K[cols], Q[rows]  # the second factors of dQ's and dK's terms
            s = float(c) * (Q[rows] * K[cols]).sum(2) + bb
        else:
            aa = np.ones(Q.shape[1:]) if gat[0] is None else np.asarray(gat[0], dtype=np.float64)
            u = Q[rows] + K[cols]
            lk = np.where(u > 0, u, float(gat[1]) * u)
            kq = qk_ = aa[None] * np.where(u > 0, 1.0, float(gat[1]))
            s = float(c) * (aa[None] * lk).sum(2) + bb
        mx = np.full((mat.m, H), -np.inf)
        np.maximum.at(mx, rows, s)
        e = np.exp(s - mx[rows])
        z = _scatter(rows, mat.m, e * (g > 0) if wrong == "z-over-kept" else e)
        p = e / z[rows]

        def side(gs):
            pg = p * gs
            dp, adp = gs * (dO[rows] * V[cols]).sum(2), gs * (np.abs(dO[rows]) * np.abs(V[cols])).sum(2)
            ds = p * (dp - _scatter(rows, mat.m, p * dp)[rows])
            ads = p * (adp + _scatter(rows, mat.m, p * adp)[rows])
            return pg, ds, ads

        pg, ds, ads = side(g)
        pgc, dsc, adsc = side(g[companion_positions(mat)]) if wrong == "mask-by-companion-position" else (pg, ds, ads)
        ac = abs(float(c))
        got = (_scatter(rows, mat.m, pg[:, :, None] * V[cols]), float(c) * _scatter(rows, mat.m, ds[:, :, None] * kq),
               float(c) * _scatter(cols, mat.n, dsc[:, :, None] * qk_), _scatter(cols, mat.n, pgc[:, :, None] * dO[rows]), ds)
        mag = (_scatter(rows, mat.m, pg[:, :, None] * np.abs(V[cols])), ac * _scatter(rows, mat.m, ads[:, :, None] * np.abs(kq)),
               ac * _scatter(cols, mat.n, adsc[:, :, None] * np.abs(qk_)), _scatter(cols, mat.n, pgc[:, :, None] * np.abs(dO[rows])),
               ads)
        if gat is not None:
            got += (float(c) * _scatter(rows, mat.m, ds[:, :, None] * lk),)
            mag += (ac * _scatter(rows, mat.m, ads[:, :, None] * np.abs(lk)),)
    return got, mag


def first_order_rho(mat, c, bias, Q, K, dtype):
    """rho' of the module docstring: edge_bias_reference's rho on the finite scores, plus the two added roundings"""
    from tests import softmax_reference as R
    from tests.exact_reference import unit_roundoff
    u = unit_roundoff(dtype)
    k = Q.shape[2]
    rows, cols = rows_cols(mat)
    Qd, Kd = (np.asarray(t, dtype=np.float64) for t in (Q, K))
    bd = np.zeros((mat.nnz, Q.shape[1])) if bias is None else np.asarray(bias, dtype=np.float64)
    finite = np.isfinite(bd)
    qk = (Qd[rows] * Kd[cols]).sum(axis=2)
    s = c * qk + np.where(finite, bd, 0.0)
    sigma_e = (k * u / (1 - k * u)) * (np.abs(Qd[rows]) * np.abs(Kd[cols])).sum(axis=2)
    sigma = float(np.where(finite, abs(c) * sigma_e + u * (np.abs(c * qk) + np.abs(np.where(finite, bd, 0.0))), 0.0).max()) if mat.nnz else 0.0
    beta = 0.0
    for h in range(s.shape[1]):  # the softmax over a row's finite entries: the pattern restricted to them
        f = finite[:, h]
        rp = np.zeros(mat.m + 1, dtype=np.int64)
        rp[1:] = np.cumsum(np.bincount(rows[f], minlength=mat.m))
        ref = R.softmax_reference(rp.astype(mat.row_ptr.dtype), s[f, h].astype(dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(ref.expected > 0, ref.bound / ref.expected, 0)
        beta = max(beta, float(np.nanmax(ratio)) if ratio.size else 0.0)
    Lmax = int(np.diff(mat.row_ptr).max()) if mat.m else 0
    scale = (1 + 2.0 ** -10) * (2 if np.dtype(dtype) == np.float64 else 1)
    return (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * scale + 2 * u * scale


def allowances(mat, c, bias, Q, K, V, dO, keep, cd, dtype, stages):
    """(rho', the reference's five outputs, their allowances): rho' mag for O, STAGES rho' mag for the gradients"""
    rho = first_order_rho(mat, c, bias, Q, K, dtype)
    got, mag = numpy_reference(mat, c, bias, Q, K, V, dO, keep, cd)
    return rho, got, (rho * mag[0],) + tuple(stages * rho * a for a in mag[1:])


def compare(got, want, allowed, what=""):
    """the worst |error| / allowance over the elements where the reference is a number; AssertionError where the reference is NaN
    and the result is not, or the other way round"""
    got, want, allowed = (np.asarray(t, dtype=np.float64) for t in (got, want, allowed))
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where the reference has none, or none where it has")
    err = np.abs(np.where(nan, 0.0, got) - np.where(nan, 0.0, want))
    ratio = err / np.maximum(np.where(nan, 1.0, allowed), 1e-300)
    return float(ratio.max()) if ratio.size else 0.0
