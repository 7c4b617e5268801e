"""csr5hip_mha_biased / csr5hip_mha_biased_backward (``A.mhaBiased``, ``A.mhaBiasedBackward``) and
``autograd.multihead_attention(..., scale, bias, slopes)`` on the GPU: softmax(scale Q K^T + slope_h A) on the pattern, A the
handle's stored values.  Tests A to E are identities that hold bit for bit; F and I go to a float64 torch reference.

WHY THE IDENTITIES HOLD.  s = fma(qk, c, b), b = slope_h * a.  (A) a = +0, c = 1: s = qk + 0, the plain score (a -0 becomes +0:
the same value, and a score enters the rest only through s - M).  (B) a = +0, c = 2**-2: s = qk / 4 exactly, which is also the
plain chain on Q / 4 (a scaling by a power of two commutes with every rounding; the uniform operands are far from the
subnormals); t = ds / 4, so dK = sum (ds / 4) Q = sum ds (Q / 4) and dQ = (sum ds K) / 4.  (C) tests/mha_bias_reference.py.
(C)'s k = 5.  TWO things must be the same for k and for the widened k + 1.  THE SUMMATION ORDER of dQ and dK is a function of
(L, width): beyond 16 entries a column block of width wb is summed in 64 / C (256 / C) slots, C the smallest power of two >= wb,
so the first k columns of a gradient of width k + 1 have the bits of a gradient of width k only where both widths round up to
the same power of two: 5 and 6 both give C = 8 (2 and 3 would give 2 and 4).  THE LOAD WIDTH: 16-byte loads need, among other
things, every row of Q and K to start on a 16-byte boundary; Q and K (and their widened forms) are passed here as views with an
ODD leading dimension (15 values in rows of 17, 18 in rows of 19), which no fp64 row alignment survives, and in fp32 k = 5 and 6
are below the one whole block of 8 values the rule asks for; the backward takes 16-byte loads only if all of Q, K, V and dO
qualify.  So the biased call and the widened plain call both take element loads, in both precisions.

(F) THE ALLOWANCE is tests/test_gpu_attention_autograd.py's (``_allowances``) with the score-error term sigma widened for the two
extra roundings.  The computed score is fl(qk^ c + b^) with qk^ the chain's result, |qk^ - qk| <= sigma_e, and b^ = fl(slope a),
|b^ - b| <= u |b|; the fused multiply-add rounds once, |fl(x) - x| <= u |x| with |x| <= |c qk^| + |b^|.  To first order
    |s^ - s| <= |c| sigma_e + u |b| + u (|c qk| + |b|) = |c| sigma_e + u (|c qk| + 2 |b|) =: sigma'_e,
and sigma' is its maximum over the entries and heads.  c is the scale in the handle's type, on both sides.  dQ and dK carry one
more rounding (t = ds c) and the factor |c|: their allowances are |c| times the plain ones, and STAGES = 8 covers the
multiplication as it covers the other stages.  dS has the allowance of ds, STAGES rho A_s.  For the gradients of bias and slopes
(I) the allowance of dS is propagated through the torch reduction: sum_h |slope_h| allow(dS[e, h]) + n u |result| resp.
sum_e |a_e| allow(dS[e, h]) plus the reduction's own gamma(n) sum |terms|."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import mha_bias_reference as B  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import softmax_reference as R  # noqa: E402
from tests import zoo  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index, _torch_softmax, _uniform, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _bits, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
POISON = -777.25
SHAPES = ((1, 8, 16), (2, 8, 16), (3, 3, 5), (2, 13, 70))


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["duplicates"] = S.duplicates_matrix()
    z["class-edges"] = E.class_edges()
    z["dealt"] = E.dealt()
    return z


def _open(mat, val, dtype, sigma=AUTO):
    return _handle(mat, np.asarray(val, dtype=dtype), Path("bias", sigma, H.SPMV_FUSED), dtype)[0]


def _operands(mat, heads, k, d, dtype, seed):
    rng = np.random.default_rng([seed, heads, k, d, 64 if dtype == np.float64 else 32])
    return (_uniform(rng, (mat.m, heads, k), dtype).mul_(2), _uniform(rng, (mat.n, heads, k), dtype),
            _uniform(rng, (mat.n, heads, d), dtype), _uniform(rng, (mat.m, heads, d), dtype))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _odd_ld(t):
    """the same (rows, heads, width) values as a view whose leading dimension is odd and above heads * width: element loads"""
    rows, w = t.shape[0], t.shape[1] * t.shape[2]
    ld = w + 2 if w % 2 else w + 1
    buf = torch.zeros((rows, ld), dtype=t.dtype, device=DEV)
    view = buf[:, :w].unflatten(1, tuple(t.shape[1:]))
    view.copy_(t)
    return view


def _nan(shape, like):
    return torch.full(tuple(shape), float("nan"), dtype=like.dtype, device=DEV)


def _plain(A, mat, Q, K, V, dO):
    """[O, dQ, dK, dV] of mha / mhaBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    assert A.mha(Q, K, V, O) == 0, _capi.last_error()
    assert A.mhaBackward(Q, K, V, dO, outs[0], outs[1], outs[2], torch.empty(4 * mat.m * Q.shape[1], dtype=Q.dtype, device=DEV)) == 0, \
        _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs


def _biased(A, mat, Q, K, V, dO, scale=1.0, slopes=None, want_dS=True):
    """[O, dQ, dK, dV, dS] of mhaBiased / mhaBiasedBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dS = _nan((mat.nnz, Q.shape[1]), Q) if want_dS else None
    assert A.mhaBiased(Q, K, V, O, scale=scale, slopes=slopes) == 0, _capi.last_error()
    work = torch.empty(4 * mat.m * Q.shape[1], dtype=Q.dtype, device=DEV)
    assert A.mhaBiasedBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, scale=scale, slopes=slopes, dS=dS) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dS]


def _same(a, b):
    return E.same_bits(a.cpu().numpy(), b.cpu().numpy())


def _written(ts, what):
    for t, n in zip(ts, ("O", "dQ", "dK", "dV", "dS")):
        assert t is None or not bool(torch.isnan(t).any()), (what, n, "an element was not written")


# ---- A. the neutral element, B. a power-of-two scale ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("half-empty", "aligned64", "aligned1024", "two-hubs"))
def test_zero_bias_is_mha_and_a_power_of_two_scale_is_mha_on_scaled_q(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, np.zeros(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    for si, (heads, k, d) in enumerate(SHAPES):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=300 + si)
        got = _biased(A, mat, Q, K, V, dO)
        _written(got, (name, heads, k, d))
        for g, w, what in zip(got, _plain(A, mat, Q, K, V, dO), ("O", "dQ", "dK", "dV")):
            assert _same(g, w), ("A", name, heads, k, d, what)
        got = _biased(A, mat, Q, K, V, dO, scale=0.25, want_dS=False)
        want = _plain(A, mat, Q * 0.25, K, V, dO)
        want[1] = want[1] * 0.25
        for g, w, what in zip(got, want, ("O", "dQ", "dK", "dV")):
            assert _same(g, w), ("B", name, heads, k, d, what)
    _close(A)


# ---- C. a real bias, exact by augmentation; G. the companion stays current ------------------------------------------------------------
def _widened(A, mat, Q, K, V, dO, u, v, slopes):
    """[O, dQ, dK, dV] expected of the biased call with the bias u[i] v[j], scale 1 and these slopes: mha / mhaBackward on Q|u, K|v"""
    dtype = np.float64 if Q.dtype == torch.float64 else np.float32
    Qw, Kw = B.augment(Q.cpu().numpy(), K.cpu().numpy(), u, v, slopes)
    k = Q.shape[2]
    O, dQw, dKw, dV = _plain(A, mat, _odd_ld(_dev(Qw, dtype)), _odd_ld(_dev(Kw, dtype)), V, dO)
    return [O, dQw[:, :, :k], dKw[:, :, :k], dV]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("sigma", (AUTO, 4), ids=("auto", "sigma4"))
@pytest.mark.parametrize("name", ("half-empty", "aligned64", "aligned1024", "two-hubs", "class-edges", "dealt"))
def test_rank_one_bias_has_the_bits_of_mha_on_widened_operands(name, sigma, dtype):
    mat = _zoo()[name]
    heads, k, d = 3, 5, 5  # (the same slot count and element loads on both sides: the module docstring)
    u, v, a = B.rank_one(mat, seed=7)
    A = _open(mat, a, dtype, sigma)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=400)
    Q, K = _odd_ld(Q), _odd_ld(K)
    for slopes in (None, (2.0, 0.5, -1.0)):
        sl = None if slopes is None else _dev(np.array(slopes), dtype)
        got = _biased(A, mat, Q, K, V, dO, slopes=sl, want_dS=False)
        _written(got, (name, slopes))
        for g, w, what in zip(got, _widened(A, mat, Q, K, V, dO, u, v, slopes), ("O", "dQ", "dK", "dV")):
            assert _same(g, w), (name, A.info().sigma, slopes, what)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_column_kernel_reads_the_companions_current_values(dtype):
    """buildTranspose, THEN updateValues, then backward: dK and dV are those of the new values"""
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        _, _, old = B.rank_one(mat, seed=8)
        u, v, new = B.rank_one(mat, seed=9)
        assert not np.array_equal(old, new)
        A = _open(mat, old, dtype, 7)
        assert A.buildTranspose() == 0, _capi.last_error()
        assert A.updateValues(_dev(new, dtype)) == 0, _capi.last_error()
        Q, K, V, dO = _operands(mat, 3, 5, 5, dtype, seed=410)
        Q, K = _odd_ld(Q), _odd_ld(K)
        got = _biased(A, mat, Q, K, V, dO, want_dS=False)
        for g, w, what in zip(got, _widened(A, mat, Q, K, V, dO, u, v, None), ("O", "dQ", "dK", "dV")):
            assert _same(g, w), (name, what)
        _close(A)


# ---- D. dS and repeated entries against the unfused chain --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("duplicates", "half-empty", "aligned1024", "class-edges"))
def test_ds_has_the_bits_of_the_unfused_chain(name, dtype):
    """per head: s = sddmm(Q_h, K_h) * scale + slopes[h] * val in torch (an exact multiplication by a power of two, one rounded
    multiplication, one rounded addition: the definition's roundings), p = rowSoftmax(s), dp = sddmm(dO_h, V_h),
    ds = rowSoftmaxGrad(p, dp); dS[:, h] must have ds's bits"""
    mat = _zoo()[name]
    rng = np.random.default_rng([500, mat.nnz])
    val = rng.uniform(-2, 2, size=mat.nnz).astype(dtype)  # (differs between the repeated pairs of the duplicates matrix)
    heads, k, d = 3, 8, 16
    A = _open(mat, val, dtype)
    vd = _dev(val, dtype)
    slopes = _dev(np.array([0.7, -1.3, 0.11]), dtype)
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=501)
    for scale in (1.0, 0.5):
        dS = _nan((mat.nnz, heads), Q)
        dQ = _nan(Q.shape, Q)
        assert A.mhaBiasedBackward(Q, K, V, dO, dQ=dQ, scale=scale, slopes=slopes, dS=dS) == 0, _capi.last_error()  # no companion, no work
        torch.cuda.synchronize()
        assert not bool(torch.isnan(dS).any()) and A.info().transpose_built == 0
        for h in range(heads):
            qk, dp, p, ds = (torch.empty(mat.nnz, dtype=Q.dtype, device=DEV) for _ in range(4))
            assert A.sddmm(Q[:, h].contiguous(), K[:, h].contiguous(), qk) == 0, _capi.last_error()
            s = qk * scale + slopes[h] * vd
            assert A.rowSoftmax(s, p) == 0 and A.sddmm(dO[:, h].contiguous(), V[:, h].contiguous(), dp) == 0, _capi.last_error()
            assert A.rowSoftmaxGrad(p, dp, ds) == 0, _capi.last_error()
            torch.cuda.synchronize()
            assert _same(dS[:, h], ds), (name, scale, h, float((dS[:, h] - ds).abs().max()))
    _close(A)


# ---- E. the mask ---------------------------------------------------------------------------------------------------------------------
def _mask(mat, seed):
    """unmasked (nnz,): every row of 17 or more entries keeps the largest power of two BELOW its length, a shorter one the largest
    power of two up to its length, every seventh non-empty short row nothing at all"""
    rng = np.random.default_rng(seed)
    keep = np.zeros(mat.nnz, dtype=bool)
    short = 0
    for i in range(mat.m):
        a, b = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
        L = b - a
        if L == 0:
            continue
        n = 1 << ((L - 1).bit_length() - 1) if L > E.AT_G else 1 << (L.bit_length() - 1)
        if L <= E.AT_G:
            short += 1
            n = 0 if short % 7 == 0 else n
        keep[a + rng.permutation(L)[:n]] = True
    return keep


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_minus_infinity_is_a_hard_mask(dtype):
    mat = _zoo()["class-edges"]
    keep = _mask(mat, 600)
    mixed, dead = E.mask_conditions(mat, keep)
    assert mixed and 0 < dead < 0.5
    heads, k, d = 2, 3, 5
    rng = np.random.default_rng(601)
    Q = torch.zeros((mat.m, heads, k), dtype=_tdt(dtype), device=DEV)  # qk = +0: the score is the bias
    K = _uniform(rng, (mat.n, heads, k), dtype)
    Vn = rng.integers(-1000, 1001, size=(mat.n, heads, d)).astype(dtype)
    dOn = rng.integers(-8, 9, size=(mat.m, heads, d)).astype(dtype)
    V, dO = _dev(Vn, dtype), _dev(dOn, dtype)
    A = _open(mat, np.where(keep, 0.0, -np.inf), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    O, dQ, dK, dV, _ = _biased(A, mat, Q, K, V, dO, scale=0.5, want_dS=False)
    _close(A)
    rows, cols = E.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    kept = np.bincount(rows[keep], minlength=mat.m)
    lens = np.diff(mat.row_ptr)
    dead_rows = (lens > 0) & (kept == 0)
    for h in range(heads):
        want, mag = E.exact_forward(mat, Vn[:, h], keep, dtype)
        assert mag < E.EXACT_LIMIT
        assert E.same_bits(O[:, h].cpu().numpy(), want), h                       # the mean of the unmasked V rows; NaN where all are masked
    assert np.array_equal(np.isnan(O.cpu().numpy()).all(axis=(1, 2)), dead_rows) and np.array_equal(np.isnan(O.cpu().numpy()).any(axis=(1, 2)), dead_rows)
    assert np.array_equal(np.isnan(dQ.cpu().numpy()).all(axis=(1, 2)), dead_rows) and np.array_equal(np.isnan(dQ.cpu().numpy()).any(axis=(1, 2)), dead_rows)
    # dV[j] = sum over the UNMASKED entries of column j of dO[i] / kept_i: dyadic, exact in every order; a masked entry adds nothing,
    # and the columns an all-masked row stores are NaN
    live = keep & ~dead_rows[rows]
    want = np.zeros((mat.n, heads, d))
    np.add.at(want, cols[live], dOn[rows[live]].astype(np.float64) / kept[rows[live]][:, None, None])
    poisoned = np.zeros(mat.n, dtype=bool)
    poisoned[cols[dead_rows[rows]]] = True
    want[poisoned] = np.nan
    assert E.same_bits(dV.cpu().numpy(), want.astype(dtype))
    assert np.array_equal(np.isnan(dK.cpu().numpy()).any(axis=(1, 2)), poisoned)


# ---- F. the float64 reference ------------------------------------------------------------------------------------------------------
def _reference(mat, rows, cols, c, val, slopes, Q, K, V, dO):
    """(O, dQ, dK, dV, dS, dval, dslopes) by torch autograd in float64"""
    Qr, Kr, Vr, ar, sr = (t.detach().double().clone().requires_grad_(True) for t in (Q, K, V, val, slopes))
    s = c * (Qr[rows] * Kr[cols]).sum(dim=2) + sr[None, :] * ar[:, None]
    s.retain_grad()
    p = torch.stack([_torch_softmax(mat, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    out = torch.zeros((mat.m,) + tuple(Vr.shape[1:]), dtype=torch.float64, device=DEV).index_add(0, rows, p[:, :, None] * Vr[cols])
    out.backward(dO.double())
    return out.detach(), Qr.grad, Kr.grad, Vr.grad, s.grad, ar.grad, sr.grad


def _bias_allowances(mat, rows, cols, c, val, slopes, Q, K, V, dO, dtype):
    """(rho, allowances of O, dQ, dK, dV, dS) in float64: ``_allowances`` with sigma' of the module docstring, per head"""
    u = unit_roundoff(dtype)
    k = Q.shape[2]
    Qd, Kd, Vd, dOd, ad, sd = (t.detach().double() for t in (Q, K, V, dO, val, slopes))
    qk = (Qd[rows] * Kd[cols]).sum(dim=2)
    b = sd[None, :] * ad[:, None]
    s = c * qk + b
    sigma_e = (k * u / (1 - k * u)) * (Qd[rows].abs() * Kd[cols].abs()).sum(dim=2)
    sigma = float((abs(c) * sigma_e + u * ((c * qk).abs() + 2 * b.abs())).max())
    beta = 0.0
    for h in range(s.shape[1]):
        ref = R.softmax_reference(mat.row_ptr, s[:, h].cpu().numpy().astype(dtype))
        with np.errstate(invalid="ignore", divide="ignore"):
            beta = max(beta, float(np.nanmax(np.where(ref.expected > 0, ref.bound / ref.expected, 0))))
    Lmax = int(np.diff(mat.row_ptr).max())
    rho = (2 * sigma + beta + Lmax * u / (1 - Lmax * u)) * (1 + 2.0 ** -10) * (2 if dtype == np.float64 else 1)
    p = torch.stack([_torch_softmax(mat, rows, s[:, h]) for h in range(s.shape[1])], dim=1)
    zeros = lambda t: torch.zeros(t.shape, dtype=torch.float64, device=DEV)  # noqa: E731
    a_out = torch.zeros((mat.m,) + tuple(Vd.shape[1:]), dtype=torch.float64, device=DEV).index_add(0, rows, p[:, :, None] * Vd[cols].abs())
    a_V = zeros(Vd).index_add(0, cols, p[:, :, None] * dOd[rows].abs())
    a_p = (dOd[rows].abs() * Vd[cols].abs()).sum(dim=2)
    a_s = p * (a_p + torch.zeros((mat.m, s.shape[1]), dtype=torch.float64, device=DEV).index_add(0, rows, p * a_p)[rows])
    a_Q = abs(c) * zeros(Qd).index_add(0, rows, a_s[:, :, None] * Kd[cols].abs())
    a_K = abs(c) * zeros(Kd).index_add(0, cols, a_s[:, :, None] * Qd[rows].abs())
    return rho, rho * a_out, STAGES * rho * a_Q, STAGES * rho * a_K, STAGES * rho * a_V, STAGES * rho * a_s


def _case_f(mat, dtype, seed):
    heads, k, d = 3, 8, 16
    rng = np.random.default_rng([seed, mat.nnz])
    val = _dev(rng.uniform(-2, 2, size=mat.nnz), dtype)
    slopes = _dev(rng.uniform(-1.5, 1.5, size=heads), dtype)
    c = float(np.asarray(1 / np.sqrt(k), dtype=dtype))  # the scale in the handle's type: what the library converts it to
    return (heads, k, d), val, slopes, c, _operands(mat, heads, k, d, dtype, seed=seed + 1)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_biased_calls_match_the_float64_reference(dtype):
    for mi, name in enumerate(("half-empty", "hub", "duplicates")):
        mat = _zoo()[name]
        rows, cols = _index(mat)
        _, val, slopes, c, (Q, K, V, dO) = _case_f(mat, dtype, 700 + 10 * mi)
        A = _open(mat, val.cpu().numpy(), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        got = _biased(A, mat, Q, K, V, dO, scale=1 / np.sqrt(8), slopes=slopes)
        _close(A)
        want = _reference(mat, rows, cols, c, val, slopes, Q, K, V, dO)
        allow = _bias_allowances(mat, rows, cols, c, val, slopes, Q, K, V, dO, dtype)
        print(f"{name} {_dt(dtype)}: rho {allow[0]:.3e}")
        assert STAGES * allow[0] <= FIRST_ORDER, (name, allow[0])
        for g, w, a, what in zip(got, want, allow[1:], ("O", "dQ", "dK", "dV", "dS")):
            _within(g, w, a, f"{name} {_dt(dtype)} {what}")


# ---- H. the contract ---------------------------------------------------------------------------------------------------------------
def _guarded(rows, width, dtype, guard=64, extra=3):
    """(buffer, view (rows, width) with leading dimension width + extra inside it, that leading dimension)"""
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
def test_only_the_outputs_are_written_and_the_handle_is_untouched(dtype):
    heads, k, d = 3, 3, 5
    for name in ("half-empty", "aligned1024", "class-edges"):
        mat = _zoo()[name]
        rng = np.random.default_rng([800, mat.nnz])
        A = _open(mat, rng.uniform(-1, 1, size=mat.nnz), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        slopes = _dev(np.array([0.5, -2.0, 1.25]), dtype)
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=801)
        keep = [t.clone() for t in (Q, K, V, dO, slopes)]
        stored, info0 = A._arrays[2].clone(), bytes(A.info())  # (the handle's own tile-ordered values: asCSR5 permuted that tensor in place)
        want = _biased(A, mat, Q, K, V, dO, scale=0.3, slopes=slopes)
        bufs = [_guarded(r, heads * w, dtype) for r, w in ((mat.m, d), (mat.m, k), (mat.n, k), (mat.n, d))] + [_guarded(mat.nnz, heads, dtype)]
        views = [b[1].unflatten(1, (heads, w)) for b, w in zip(bufs[:4], (d, k, k, d))] + [bufs[4][1]]
        assert A.mhaBiased(Q, K, V, views[0], scale=0.3, slopes=slopes) == 0, _capi.last_error()
        work = torch.empty(4 * mat.m * heads, dtype=Q.dtype, device=DEV)
        assert A.mhaBiasedBackward(Q, K, V, dO, views[1], views[2], views[3], work, scale=0.3, slopes=slopes, dS=views[4]) == 0, \
            _capi.last_error()
        torch.cuda.synchronize()
        for (b, _, ld), w, width, rws in zip(bufs, want, (heads * d, heads * k, heads * k, heads * d, heads),
                                             (mat.m, mat.m, mat.n, mat.n, mat.nnz)):
            body = _guard_intact(b, rws, width, ld)
            assert np.array_equal(_bits(body), _bits(w.reshape(rws, -1).cpu().numpy())), name
        for t, k0 in zip((Q, K, V, dO, slopes), keep):
            assert torch.equal(t, k0)
        assert torch.equal(A._arrays[2], stored) and bytes(A.info()) == info0
        # nothing wanted: a successful no-op, with or without operands
        assert A.mhaBiasedBackward(Q, K, V, dO, scale=0.3, slopes=slopes) == 0, _capi.last_error()
        assert A.mha_biased_backward_ptr(heads, 0.3, None, None, 9, None, 9, k, None, 15, d, None, 15, None, 9, None, 9, None, 15, None, None,
                                         3) == 0, _capi.last_error()
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_degenerate_shapes_and_the_error_order(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    Q, K, V, dO = _operands(mat, 3, 4, 6, dtype, seed=810)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    dS = torch.full((mat.nnz, 3), POISON, dtype=_tdt(dtype), device=DEV)
    INV = _capi.INVALID_ARGUMENT
    assert A.mha_biased_ptr(0, 1.0, None, Q, 12, K, 12, 4, V, 18, 6, O, 18) == 0, _capi.last_error()  # heads = 0
    assert A.mha_biased_ptr(3, 1.0, None, Q, 12, K, 12, 4, V, 18, 0, O, 18) == 0, _capi.last_error()  # d = 0
    assert A.mha_biased_backward_ptr(0, 1.0, None, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, dS, 3) == 0
    torch.cuda.synchronize()
    assert bool((O == POISON).all()) and bool((dS == POISON).all())
    # the scale and ldds are rejected on a converted handle too (their place in the order: tests/test_mha_bias_host.py)
    assert A.mha_biased_ptr(3, float("nan"), None, None, 0, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.mha_biased_backward_ptr(3, float("inf"), None, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, K, 12, None, 18, None, dS, 3) == INV
    assert A.mha_biased_backward_ptr(3, 1.0, None, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, dS, 2) == INV
    dK = torch.empty_like(K)
    assert A.mhaBiasedBackward(Q, K, V, dO, dK=dK, work=torch.empty(12 * mat.m, dtype=Q.dtype, device=DEV)) == INV  # no companion
    assert "transposed companion" in _capi.last_error()
    # d = 0 in the backward: dS is the score gradient of an empty product, +0 wherever p is finite
    V0, dO0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.n, mat.m))
    assert A.mhaBiasedBackward(Q, K, V0, dO0, dS=dS) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not _bits(dS.cpu().numpy()).any()
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0: +0 everywhere, no element of dS
    A = _open(none, np.zeros(0), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(none, 3, 4, 6, dtype, seed=811)
    for t in _biased(A, none, Q, K, V, dO, scale=2.0):
        assert not _bits(t.cpu().numpy()).any()
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_both_calls_replay_from_a_graph(dtype):
    """one forward and one backward, captured on a single linear stream that has run them once before"""
    mat = _zoo()["half-empty"]
    rng = np.random.default_rng(820)
    A = _open(mat, rng.uniform(-1, 1, size=mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    slopes = _dev(np.array([1.0, -0.5, 0.25]), dtype)
    Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=821)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    outs = [torch.full(t.shape, POISON, dtype=t.dtype, device=DEV) for t in (Q, K, V)]
    dS = torch.full((mat.nnz, 3), POISON, dtype=_tdt(dtype), device=DEV)
    work = torch.empty(12 * mat.m, dtype=Q.dtype, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0

    def both():
        assert A.mhaBiased(Q, K, V, O, scale=0.4, slopes=slopes) == 0, _capi.last_error()
        assert A.mhaBiasedBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, scale=0.4, slopes=slopes, dS=dS) == 0, _capi.last_error()
    with torch.cuda.stream(side):
        both()  # (the stream has run the calls once before the capture)
    torch.cuda.synchronize()
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    Qn = _operands(mat, 3, 5, 6, dtype, seed=822)[0]
    Q.copy_(Qn)  # changed in place: the graph reads the same address
    for t in [O] + outs + [dS]:
        t.fill_(POISON)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in [O] + outs + [dS]]
    del graph
    assert A.setStream(None) == 0
    for g, e in zip(replayed, _biased(A, mat, Qn, K, V, dO, scale=0.4, slopes=slopes)):
        assert _same(g, e)
    _close(A)


# ---- I. autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_autograd_gradients_match_the_float64_reference(dtype):
    u = unit_roundoff(dtype)
    for mi, name in enumerate(("half-empty", "duplicates")):
        mat = _zoo()[name]
        rows, cols = _index(mat)
        (heads, _, _), val, slopes, c, (Q, K, V, dO) = _case_f(mat, dtype, 900 + 10 * mi)
        A = _open(mat, np.ones(mat.nnz), dtype)
        q, k_, v, a, sl = (t.clone().requires_grad_(True) for t in (Q, K, V, val, slopes))
        out = autograd.multihead_attention(A, q, k_, v, scale=1 / np.sqrt(8), bias=a, slopes=sl)
        other = autograd.multihead_attention(A, Q, K, V, bias=val * 2)  # another forward replaces the handle's values in between
        out.backward(dO)
        torch.cuda.synchronize()
        del other
        _close(A)
        want = _reference(mat, rows, cols, c, val, slopes, Q, K, V, dO)
        rho, a_O, a_Q, a_K, a_V, a_S = _bias_allowances(mat, rows, cols, c, val, slopes, Q, K, V, dO, dtype)
        assert STAGES * rho <= FIRST_ORDER
        for g, w, al, what in zip((out.detach(), q.grad, k_.grad, v.grad), want[:4], (a_O, a_Q, a_K, a_V), ("O", "dQ", "dK", "dV")):
            _within(g, w, al, f"{name} {_dt(dtype)} {what}")
        sd, ad, dSr = slopes.double(), val.double(), want[4]
        gam = lambda n: n * u / (1 - n * u)  # noqa: E731
        a_bias = (a_S * sd.abs()[None, :]).sum(1) + gam(heads + 1) * (dSr.abs() * sd.abs()[None, :]).sum(1)
        a_slopes = (a_S * ad.abs()[:, None]).sum(0) + gam(mat.nnz + 1) * (dSr.abs() * ad.abs()[:, None]).sum(0)
        _within(a.grad, want[5], a_bias, f"{name} {_dt(dtype)} dbias")
        _within(sl.grad, want[6], a_slopes, f"{name} {_dt(dtype)} dslopes")


def test_autograd_without_the_new_arguments_is_todays_call_and_the_handle_holds_the_bias():
    mat = _zoo()["half-empty"]
    dtype = np.float64
    A = _open(mat, np.ones(mat.nnz), dtype)
    Q, K, V, dO = _operands(mat, 3, 8, 5, dtype, seed=950)
    q, k_, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    autograd.multihead_attention(A, q, k_, v, None, None, None).backward(dO)
    torch.cuda.synchronize()
    assert getattr(A, "_autograd_key", None) is None                          # today's path: the record of the values untouched
    want = _plain(A, mat, Q, K, V, dO)
    assert _same(autograd.multihead_attention(A, Q, K, V).detach(), want[0])
    for g, w in zip((q.grad, k_.grad, v.grad), want[1:]):
        assert _same(g, w)
    bias = _dev(np.random.default_rng(951).uniform(-1, 1, size=mat.nnz), dtype)
    out = autograd.multihead_attention(A, Q, K, V, bias=bias)                  # scale None = 1.0, no slopes
    assert A._autograd_key is not None and A._autograd_val.data_ptr() == bias.data_ptr()   # the handle now holds the bias
    assert _same(out, _biased(A, mat, Q, K, V, dO, want_dS=False)[0])
    held = autograd.multihead_attention(A, Q, K, V, scale=1.0)                 # bias None: whatever the handle holds
    assert _same(held, out)
    # bias None keeps nothing to give again: a forward that replaces the handle's values in between makes backward raise
    q = Q.clone().requires_grad_(True)
    first = autograd.multihead_attention(A, q, K, V, scale=1.0)
    autograd.multihead_attention(A, Q, K, V, bias=bias * 2)
    with pytest.raises(RuntimeError, match="values were replaced"):
        first.backward(dO)
    q2 = Q.clone().requires_grad_(True)                                       # undisturbed, the same backward goes through
    autograd.multihead_attention(A, q2, K, V, scale=1.0).backward(dO)
    torch.cuda.synchronize()
    assert q2.grad is not None and not bool(torch.isnan(q2.grad).any())
    _close(A)
