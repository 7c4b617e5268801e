"""csr5hip_dropout_mha / csr5hip_dropout_gat, their backwards and csr5hip_dropout_mask (``A.dropoutMha`` ..., ``A.dropoutMask``) and
``autograd.dropout_attention`` / ``autograd.gat_dropout_attention`` on the GPU.  Tests 1 to 4 and 6 are identities that hold bit
for bit; 5 goes to the numpy float64 reference under the allowance of tests/dropout_reference.py.

WHY THE IDENTITIES HOLD.  (1) the mask is a pure integer function, restated in numpy.  (2) p = 0 gives thr = 0 and cd = 1: every
weight is kept, rinv * 1 and 1 * dp and p * 1 are their operands' bits.  (3) Q = +0 makes every score +0, every weight 1 and Z = L
exactly; with p = 1/2, cd = 2 and small integer V the product's accumulator is an exact integer in every summation order, and
O = fl(acc * (fl(1 / L) * 2)) is one rounding.  For the backward a bias of {+0, -Inf} leaves a power of two n <= 16 of finite
entries in every row, so p_e = 1 / n on ANY pattern -- ``dealt``, its transpose and duplicates --, g in {0, 2}, and dp, n D and
n^2 ds are integers: with Q = +0 dQ, with K = +0 dK, and dV and dB are exact in every order, through the column kernel's map too.
(4) the mask of absolute head head0 + h does not depend on how the heads are packed.  (6) the additive call's score is restated by
tests/gat_reference.py ``scores``; ``dropoutMha`` with k = 0 and B' those scores runs the dropped EDGE code on the same scores."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import dropout_reference as DR  # noqa: E402
from tests import edge_bias_reference as EB  # noqa: E402
from tests import gat_reference as G  # noqa: E402
from tests import handle_history as HH  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _uniform  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _bits, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
POISON = -777.25
SEED, OFFSET = 2 ** 63 + 5, 2 ** 32 + 1
NAMES = DR.NAMES
GNAMES = G.NAMES


def _tdt(dtype):
    return torch.float64 if dtype == np.float64 else torch.float32


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


@functools.lru_cache(maxsize=1)
def _zoo():
    z = {m.name: m for m in zoo.small_zoo()}
    z["duplicates"] = S.duplicates_matrix()
    z["class-edges"] = E.class_edges()
    z["class-edges^T"] = EB.transposed(z["class-edges"])
    z["dealt"] = E.dealt()
    return z


def _open(mat, val, dtype, sigma=AUTO):
    A = _handle(mat, np.asarray(val, dtype=dtype), Path("dropout", sigma, H.SPMV_FUSED), dtype)[0]
    assert A.buildTranspose() == 0, _capi.last_error()
    return A


def _operands(mat, heads, k, d, dtype, seed):
    rng = np.random.default_rng([seed, heads, k, d, 64 if dtype == np.float64 else 32])
    return (_uniform(rng, (mat.m, heads, k), dtype).mul_(2), _uniform(rng, (mat.n, heads, k), dtype),
            _uniform(rng, (mat.n, heads, d), dtype), _uniform(rng, (mat.m, heads, d), dtype))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _nan(shape, like):
    return torch.full(tuple(shape), float("nan"), dtype=like.dtype, device=DEV)


def _work(mat, Q):
    return torch.empty(4 * mat.m * Q.shape[1], dtype=Q.dtype, device=DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return E.same_bits(_np(a), _np(b))


def _drop(A, mat, Q, K, V, dO, p, seed=SEED, offset=OFFSET, head0=0, Bt=None, scale=1.0):
    """[O, dQ, dK, dV, dB] of dropoutMha / dropoutMhaBackward, every output pre-filled with NaN"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dB = _nan((mat.nnz, Q.shape[1]), Q)
    assert A.dropoutMha(Q, K, V, O, p, seed, offset, head0, B=Bt, scale=scale) == 0, _capi.last_error()
    assert A.dropoutMhaBackward(Q, K, V, dO, p, seed, offset, head0, dQ=outs[0], dK=outs[1], dV=outs[2], work=_work(mat, Q), B=Bt,
                                scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dB]


def _edge(A, mat, Q, K, V, dO, Bt=None, scale=1.0):
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dB = _nan((mat.nnz, Q.shape[1]), Q)
    assert A.mhaEdgeBias(Q, K, V, O, B=Bt, scale=scale) == 0, _capi.last_error()
    assert A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q), B=Bt, scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dB]


def _gat(A, mat, Q, K, V, dO, a, ns, Bt, scale, drop=None):
    """[O, dQ, dK, dV, dB, dAr] of gat / gatBackward (drop None) or of dropoutGat / dropoutGatBackward (drop = (p, seed, offset, head0))"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dB, dAr = _nan((mat.nnz, Q.shape[1]), Q), _nan(Q.shape, Q)
    kw = dict(a=a, negative_slope=ns, B=Bt, scale=scale)
    if drop is None:
        assert A.gat(Q, K, V, O, **kw) == 0, _capi.last_error()
        assert A.gatBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q), dB=dB, dAr=dAr, **kw) == 0, _capi.last_error()
    else:
        assert A.dropoutGat(Q, K, V, O, *drop, **kw) == 0, _capi.last_error()
        assert A.dropoutGatBackward(Q, K, V, dO, *drop, dQ=outs[0], dK=outs[1], dV=outs[2], work=_work(mat, Q), dB=dB, dAr=dAr,
                                    **kw) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dB, dAr]


def _written(ts, what):
    for t, n in zip(ts, GNAMES):
        assert not bool(torch.isnan(t).any()), (what, n, "an element was not written")


# ---- 1. the mask ----------------------------------------------------------------------------------------------------------------------
def test_the_mask_is_the_reference_byte_for_byte():
    mat = _zoo()["class-edges"]
    assert mat.nnz > 2 ** 16
    A = _open(mat, np.ones(mat.nnz), np.float32)
    for heads in (1, 3, 4, 5, 8):
        for head0 in (0, 3):
            for p in (0.0, 0.1, 0.5, 0.6):
                wide = torch.full((mat.nnz, heads + 3), 0xAB, dtype=torch.uint8, device=DEV)   # ldm > heads: three guard bytes a row
                assert A.dropoutMask(wide[:, :heads], p, SEED, OFFSET, head0) == 0, _capi.last_error()
                torch.cuda.synchronize()
                got = _np(wide)
                assert np.array_equal(got[:, :heads], DR.mask(mat.nnz, heads, p, SEED, OFFSET, head0)), (heads, head0, p)
                assert (got[:, heads:] == 0xAB).all(), (heads, head0, p, "guard bytes")
    _close(A)
    # a handle in CSR format: the mask needs only nnz
    rp, ci, va = (torch.from_numpy(t).to(DEV) for t in (mat.row_ptr.astype(np.int32), mat.col.astype(np.int32), np.ones(mat.nnz)))
    A = H.anonymouslibHandle(mat.m, mat.n, dtype="float64")
    A._arrays = (rp, ci, va)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0
    m = torch.full((mat.nnz, 5), 7, dtype=torch.uint8, device=DEV)
    assert A.dropoutMask(m, 0.6, 3, 4) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_np(m), DR.mask(mat.nnz, 5, 0.6, 3, 4))
    A.close()


# ---- 2. p = 0 is the undropped sibling, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("kat0", "half-empty", "aligned64", "aligned1024", "two-hubs", "duplicates", "class-edges", "class-edges^T",
                                  "dealt"))
def test_p_zero_has_the_bits_of_the_undropped_calls(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, np.full(mat.nnz, 3.5), dtype)
    for si, (heads, k, d) in enumerate(((1, 16, 16), (3, 3, 5), (2, 13, 70))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, 3100 + si)
        Bt = _dev(EB.distinct_bias(mat, heads, 3110 + si), dtype) if si != 0 else None
        got, want = _drop(A, mat, Q, K, V, dO, 0.0, Bt=Bt, scale=0.3), _edge(A, mat, Q, K, V, dO, Bt, 0.3)
        for g, w, n in zip(got, want, NAMES):
            assert _same(g, w), (name, _dt(dtype), heads, k, d, n)
        a = _dev(np.random.default_rng(3120 + si).uniform(-1, 1, size=(heads, k)), dtype)
        got, want = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(0.0, SEED, OFFSET, 2)), _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3)
        _written(got, name)
        for g, w, n in zip(got, want, GNAMES):
            assert _same(g, w), (name, _dt(dtype), heads, k, d, "gat", n)
    _close(A)


# ---- 3. exact expectations in every summation order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_exact_forward_on_every_row_class(dtype):
    """class-edges, Q = +0, p = 1/2: O = (sum of the kept V rows) * (fl(1 / L) * 2), one wrong mask bit in any row changes it"""
    mat = _zoo()["class-edges"]
    rows, cols = DR.rows_cols(mat)
    heads, k, d = 3, 3, 5
    rng = np.random.default_rng([3200, 64 if dtype == np.float64 else 32])
    Vn = rng.integers(1, 8, size=(mat.n, heads, d)) * rng.choice((-1, 1), size=(mat.n, heads, d))
    A = _open(mat, np.ones(mat.nnz), dtype)
    Q = torch.zeros((mat.m, heads, k), dtype=_tdt(dtype), device=DEV)
    K = _uniform(rng, (mat.n, heads, k), dtype)
    O = _nan((mat.m, heads, d), Q)
    assert A.dropoutMha(Q, K, _dev(Vn, dtype), O, 0.5, SEED, OFFSET, 1) == 0, _capi.last_error()
    torch.cuda.synchronize()
    _close(A)
    keep = DR.mask(mat.nnz, heads, 0.5, SEED, OFFSET, 1).astype(np.int64)
    acc = np.zeros((mat.m, heads, d), dtype=np.int64)
    np.add.at(acc, rows, keep[:, :, None] * Vn[cols])
    L = np.diff(mat.row_ptr).astype(np.int64)
    assert np.abs(acc).max() < E.EXACT_LIMIT
    with np.errstate(divide="ignore", invalid="ignore"):
        rinv = (dtype(1) / L.astype(dtype)) * DR.cd_of(0.5, dtype)
        want = np.where((L > 0)[:, None, None], acc.astype(dtype) * rinv[:, None, None], dtype(0)).astype(dtype)
    assert E.same_bits(_np(O), want)
    assert (keep.sum(0) > 0).all() and (keep.sum(0) < mat.nnz).all()


def _power_of_two_finite(mat, heads, seed):
    """finite (nnz, heads) bool: in every non-empty row and head n = the largest power of two up to min(L, 16) entries, chosen at
    random, are finite; the others get a bias of -Inf.  Z = n and p_e = 1 / n are then exact on ANY pattern"""
    rng = np.random.default_rng(seed)
    finite = np.zeros((mat.nnz, heads), dtype=bool)
    for i in range(mat.m):
        a, b = int(mat.row_ptr[i]), int(mat.row_ptr[i + 1])
        if b > a:
            n = 1 << (min(b - a, 16).bit_length() - 1)
            for h in range(heads):
                finite[a + rng.permutation(b - a)[:n], h] = True
    return finite


@functools.lru_cache(maxsize=None)
def _exact_pattern(name):
    return EB.transposed(_zoo()["dealt"]) if name == "dealt^T" else _zoo()[name]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("zero", ("Q", "K"))
@pytest.mark.parametrize("name", ("dealt", "dealt^T", "duplicates"))
def test_exact_backward_through_the_column_kernels_map(name, zero, dtype):
    """dealt (16 entries in every row, columns of every class), its transpose (rows of every class, 16 entries in every column) and
    duplicates.  A bias of {+0, -Inf} leaves a power of two n <= 16 of finite entries in every row and head; the zero operand (Q or
    K) makes every finite score +0: p_e = 1 / n exactly.  K (or Q), V and dO are small integers that differ from entry to entry,
    p = 1/2, so g in {0, 2}: dp, n D and n^2 ds are integers, every term of every output a multiple of 1/256 (1/16 for O and dV),
    and the sums of absolute terms stay below 2^24 units: EVERY OUTPUT IS EXACT IN EVERY SUMMATION ORDER.  zero = "Q": dQ is the
    non-trivial one of (dQ, dK); zero = "K": dK is -- ds through the column kernel's map, with g indexed by map[position].  The
    expectation is tests/dropout_reference.py's float64 formulas, which are exact on these dyadic numbers."""
    mat = _exact_pattern(name)
    heads, k, d = 2, 3, 5
    rng = np.random.default_rng([3300, 64 if dtype == np.float64 else 32, zero == "K"])
    Xn = rng.integers(-2, 3, size=(mat.n if zero == "Q" else mat.m, heads, k))
    Qn = np.zeros((mat.m, heads, k), dtype=np.int64) if zero == "Q" else Xn
    Kn = Xn if zero == "Q" else np.zeros((mat.n, heads, k), dtype=np.int64)
    Vn, dOn = rng.integers(-2, 3, size=(mat.n, heads, d)), rng.integers(-2, 3, size=(mat.m, heads, d))
    finite = _power_of_two_finite(mat, heads, 3310)
    bias = np.where(finite, 0.0, -np.inf)
    keep = DR.mask(mat.nnz, heads, 0.5, SEED, OFFSET, 2)
    want, mag = DR.numpy_reference(mat, 1.0, bias, Qn, Kn, Vn, dOn, keep, 2.0)
    for w, m_, unit, n in zip(want, mag, (16, 256, 256, 16, 256), NAMES):
        assert not np.isnan(w).any() and np.array_equal(w * unit, np.rint(w * unit)), (n, "a multiple of the unit")
        assert m_.max() * unit < E.EXACT_LIMIT, (n, float(m_.max() * unit))     # exact in every order, in fp32 too
    A = _open(mat, np.ones(mat.nnz), dtype)
    got = [_np(t) for t in _drop(A, mat, _dev(Qn, dtype), _dev(Kn, dtype), _dev(Vn, dtype), _dev(dOn, dtype), 0.5, head0=2,
                                 Bt=_dev(bias, dtype))]
    _close(A)
    for g, w, n in zip(got, want, NAMES):
        assert np.array_equal(g, w.astype(dtype)), (name, zero, n, _dt(dtype))  # (values: a zero of either sign is the zero)
    moving = want[1] if zero == "Q" else want[2]
    assert moving.any() and want[4].any() and want[3].any() and (keep == 0).any() and (keep == 1).any()
    if name != "dealt":
        assert (~finite).any()                                                   # -Inf entries: rows that are no power of two



# ---- 4. packed against head by head ------------------------------------------------------------------------------------------------
def _head_by_head(A, mat, heads, k, d, dtype, seed, p):
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed)
    Bt = _dev(EB.distinct_bias(mat, heads, seed + 1), dtype)
    a = _dev(np.random.default_rng(seed + 2).uniform(-1, 1, size=(heads, k)), dtype)
    packed = _drop(A, mat, Q, K, V, dO, p, head0=1, Bt=Bt, scale=0.3)
    gpacked = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(p, SEED, OFFSET, 1))
    for h in range(heads):
        sl = slice(h, h + 1)
        one = _drop(A, mat, Q[:, sl], K[:, sl], V[:, sl], dO[:, sl], p, head0=1 + h, Bt=Bt[:, sl], scale=0.3)
        for g, w, n in zip(packed, one, NAMES):
            assert _same(g[:, sl].contiguous(), w), (mat.name, _dt(dtype), heads, n, "head", h)
        gone = _gat(A, mat, Q[:, sl], K[:, sl], V[:, sl], dO[:, sl], a[sl], 0.2, Bt[:, sl], 0.3, drop=(p, SEED, OFFSET, 1 + h))
        for g, w, n in zip(gpacked, gone, GNAMES):
            assert _same(g[:, sl].contiguous(), w), (mat.name, _dt(dtype), heads, "gat", n, "head", h)
    return packed


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("heads", (3, 5))
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T"))
def test_every_head_is_the_single_head_call_with_its_absolute_head(name, heads, dtype):
    mat = _zoo()[name]
    A = _open(mat, np.ones(mat.nnz), dtype)
    packed = _head_by_head(A, mat, heads, 3, 5, dtype, 3400 + heads, 0.6)
    _written(packed, name)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("lines,per_group", ((90113, 3), (262145, 8)), ids=("3+3+2", "one-group"))
def test_eight_heads_in_wide_groups(lines, per_group, dtype):
    assert E.heads_per_group(lines, 8) == per_group
    mat = E.many_lines(lines)
    A = _open(mat, np.ones(mat.nnz), dtype)
    _head_by_head(A, mat, 8, 3, 5, dtype, 3450, 0.1)
    _close(A)


# ---- 5. the float64 reference ------------------------------------------------------------------------------------------------------
def _reference_case(mat, dtype, p, seed, masked):
    heads, k, d = EB.F_HEADS, EB.F_K, EB.F_D
    bias, c, (Q, K, V, dO) = EB.case(mat, heads, k, d, dtype, seed)
    if masked:  # -Inf entries in every head, and one row masked entirely in head 1
        rng = np.random.default_rng(seed + 9)
        bias[rng.random(bias.shape) < 0.1] = -np.inf
        L = np.diff(mat.row_ptr)
        row = int(np.flatnonzero(L >= 3)[5])
        bias[mat.row_ptr[row]:mat.row_ptr[row + 1], 1] = -np.inf
        live = np.ones(mat.m, dtype=bool)
        live[row] = False
        for h in range(heads):  # (no other row is dead in any head: at least one finite entry each)
            first = mat.row_ptr[:-1][(L > 0) & (live | (h != 1))]
            bias[first, h] = 0.0
    A = _open(mat, np.full(mat.nnz, 3.5), dtype)
    dev = [_dev(t, dtype) for t in (Q, K, V, dO)]
    got = [_np(t) for t in _drop(A, mat, *dev, p, seed=seed, offset=7, head0=2, Bt=_dev(bias, dtype), scale=c)]
    _close(A)
    keep, cd = DR.mask(mat.nnz, heads, p, seed, 7, 2), DR.cd_of(p, dtype)
    rho, want, allow = DR.allowances(mat, c, bias, Q, K, V, dO, keep, cd, dtype, STAGES)
    assert STAGES * rho <= FIRST_ORDER, rho
    worst = {}
    for g, w, al, n in zip(got, want, allow, NAMES):
        worst[n] = DR.compare(g, w, al, n)
        print(f"{mat.name} {_dt(dtype)} p={p} masked={masked} {n}: worst |error| / allowance {worst[n]:.3f}")
    if masked:
        assert np.isnan(want[0][:, 1]).any() and not np.isnan(want[0][:, 0]).any() and not np.isnan(want[0][:, 2]).any()
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("p", (0.1, 0.6))
@pytest.mark.parametrize("which", ("class-edges", "random", "class-edges^T"))
def test_the_float64_reference_forward_and_every_gradient(which, p, dtype):
    mat = EB.random_matrix() if which == "random" else _zoo()[which]
    _reference_case(mat, dtype, p, 3500 + int(10 * p), masked=False)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("p", (0.1, 0.6))
def test_the_float64_reference_with_minus_infinity_in_the_bias(p, dtype):
    _reference_case(EB.random_matrix(), dtype, p, 3550 + int(10 * p), masked=True)
    _reference_case(_zoo()["duplicates"], dtype, p, 3560 + int(10 * p), masked=False)


# ---- 6. the additive call through the dropped edge code ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("two-hubs", "duplicates", "class-edges", "class-edges^T", "dealt"))
def test_dropped_gat_against_dropped_mha_on_the_restated_scores(name, dtype):
    """O, dV and dB bit for bit against dropoutMha with k = 0 and B' the numpy scores; dQ, dK and dAr against the call's own dB per
    line under gamma(L + 2) (tests/test_gpu_gat.py's (3)); a = None against ones"""
    mat = _zoo()[name]
    rows, cols = G.rows_cols(mat)
    A = _open(mat, np.full(mat.nnz, 3.5), dtype)
    u = unit_roundoff(dtype)
    ld = np.longdouble
    drop = (0.6, SEED, OFFSET, 3)
    for si, (heads, k, d, a_given) in enumerate(((3, 3, 5, True), (5, 1, 5, False))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, 3600 + si)
        an = G.exact_a(heads, k, dtype) if a_given else None
        bn = EB.distinct_bias(mat, heads, 3610 + si).astype(dtype)
        at = _dev(an, dtype) if a_given else None
        got = _gat(A, mat, Q, K, V, dO, at, 0.2, _dev(bn, dtype), 0.25, drop=drop)
        _written(got, name)
        s = G.scores(mat, _np(Q), _np(K), an, 0.2, 0.25, bn, dtype)
        Q0, K0 = (torch.zeros((r, heads, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))
        want = _drop(A, mat, Q0, K0, V, dO, *drop, Bt=_dev(s, dtype), scale=1.0)
        for g, w, n in zip((got[0], got[3], got[4]), (want[0], want[3], want[4]), ("O", "dV", "dB")):
            assert _same(g, w), (name, _dt(dtype), heads, k, n)
        if not a_given:
            ones = _gat(A, mat, Q, K, V, dO, torch.ones((heads, k), dtype=Q.dtype, device=DEV), 0.2, _dev(bn, dtype), 0.25, drop=drop)
            for g, w, n in zip(got, ones, GNAMES):
                assert _same(g, w), (name, n, "a = None against ones")
        gn = [_np(t) for t in got]
        ns, c = dtype(0.2), dtype(0.25)
        uu = _np(Q)[rows] + _np(K)[cols]
        t = gn[4].astype(ld) * ld(c)
        gg = np.where(uu > 0, ld(1), ld(ns))
        w_ = gg if an is None else an.astype(ld)[None] * gg
        l_ = np.where(uu > 0, uu.astype(ld), ld(ns) * uu.astype(ld))
        for what, gi, idx, lines, second in (("dQ", 1, rows, mat.m, w_), ("dK", 2, cols, mat.n, w_), ("dAr", 5, rows, mat.m, l_)):
            ref, mag = np.zeros((lines, heads, k), dtype=ld), np.zeros((lines, heads, k), dtype=ld)
            np.add.at(ref, idx, t[:, :, None] * second)
            np.add.at(mag, idx, np.abs(t)[:, :, None] * np.abs(second))
            L = np.bincount(idx, minlength=lines).astype(np.float64) + 2
            gamma = (L * u / (1 - L * u))[:, None, None]
            err = np.abs(gn[gi].astype(ld) - ref)
            assert (err <= gamma * mag).all(), (name, _dt(dtype), heads, k, what, float((err / np.maximum(gamma * mag, 1e-300)).max()))
    _close(A)


# ---- 7. contracts -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_determinism_single_outputs_guards_and_the_untouched_handle(dtype):
    mat = _zoo()["two-hubs"]
    val = np.full(mat.nnz, np.nan)                                             # NaN in the handle's values: they are not read
    A = _open(mat, val, dtype)
    info = bytes(A.info())
    heads, k, d = 3, 3, 5
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, 3700)
    Bt = _dev(EB.distinct_bias(mat, heads, 3701), dtype)
    a = _dev(np.random.default_rng(3702).uniform(-1, 1, size=(heads, k)), dtype)
    first, again = _drop(A, mat, Q, K, V, dO, 0.6, Bt=Bt, scale=0.3), _drop(A, mat, Q, K, V, dO, 0.6, Bt=Bt, scale=0.3)
    other = _drop(A, mat, Q, K, V, dO, 0.6, offset=OFFSET + 1, Bt=Bt, scale=0.3)
    for f, g, o, n in zip(first, again, other, NAMES):
        assert not bool(torch.isnan(f).any()), n
        assert _same(f, g), (n, "the same seed and offset")
        assert not _same(f, o), (n, "another offset")
    gfirst = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(0.6, SEED, OFFSET, 0))
    assert not _same(gfirst[0], _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(0.6, SEED + 1, OFFSET, 0))[0])
    # each output alone; the row side without companion and workspace
    for i, n in enumerate(("dQ", "dK", "dV", "dB")):
        out = _nan(first[i + 1].shape, Q)
        kw = {n: out}
        if n in ("dK", "dV"):
            kw["work"] = _work(mat, Q)
        assert A.dropoutMhaBackward(Q, K, V, dO, 0.6, SEED, OFFSET, B=Bt, scale=0.3, **kw) == 0, _capi.last_error()
        torch.cuda.synchronize()
        assert _same(out, first[i + 1]), n
    for i, n in ((1, "dQ"), (4, "dB"), (5, "dAr")):
        out = _nan(gfirst[i].shape, Q)
        assert A.dropoutGatBackward(Q, K, V, dO, 0.6, SEED, OFFSET, a=a, B=Bt, scale=0.3, **{n: out}) == 0, _capi.last_error()
        torch.cuda.synchronize()
        assert _same(out, gfirst[i]), ("gat", n)
    # guard words and NaN in all padding: operands as slices of wider, NaN-filled tensors; outputs with guard columns
    pad = lambda t, w: torch.full((t.shape[0], heads * t.shape[2] + w), float("nan"), dtype=t.dtype, device=DEV)  # noqa: E731

    def padded(t, w=3):
        wide = pad(t, w)
        view = wide[:, :heads * t.shape[2]].unflatten(1, (heads, t.shape[2]))
        view.copy_(t)
        return wide, view
    (_, Qp), (_, Kp), (_, Vp), (_, dOp) = (padded(t) for t in (Q, K, V, dO))
    Bw = torch.full((mat.nnz, heads + 2), float("nan"), dtype=Q.dtype, device=DEV)
    Bw[:, :heads] = Bt
    guards = []
    outs = []
    for t in (first[0], Q, K, V):
        wide = torch.full((t.shape[0], heads * t.shape[2] + 3), POISON, dtype=t.dtype, device=DEV)
        guards.append(wide)
        outs.append(wide[:, :heads * t.shape[2]].unflatten(1, (heads, t.shape[2])))
    dBw = torch.full((mat.nnz, heads + 2), POISON, dtype=Q.dtype, device=DEV)
    assert A.dropoutMha(Qp, Kp, Vp, outs[0], 0.6, SEED, OFFSET, B=Bw[:, :heads], scale=0.3) == 0, _capi.last_error()
    assert A.dropoutMhaBackward(Qp, Kp, Vp, dOp, 0.6, SEED, OFFSET, dQ=outs[1], dK=outs[2], dV=outs[3], work=_work(mat, Q), B=Bw[:, :heads],
                                scale=0.3, dB=dBw[:, :heads]) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for o, f, wide, n in zip(outs + [dBw[:, :heads]], first, guards + [dBw], NAMES):
        assert _same(o.contiguous(), f), (n, "padded")
        assert bool((wide[:, -2:] == POISON).all()), (n, "guard words")
    assert bytes(A.info()) == info and bool(torch.isnan(A._arrays[2]).all())
    _close(A)
    # the row side needs neither companion nor workspace
    C_ = _handle(mat, np.asarray(val, dtype=dtype), Path("dropout-row", AUTO, H.SPMV_FUSED), dtype)[0]
    dQ, dB = _nan(Q.shape, Q), _nan(Bt.shape, Bt)
    assert C_.dropoutMhaBackward(Q, K, V, dO, 0.6, SEED, OFFSET, dQ=dQ, B=Bt, scale=0.3, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert C_.info().transpose_built == 0 and _same(dQ, first[1]) and _same(dB, first[4])
    _close(C_)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_degenerate_shapes(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    Q, K, V, dO = _operands(mat, 3, 4, 6, dtype, seed=3740)
    Bt = _dev(EB.distinct_bias(mat, 3, 3741), dtype)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    INV = _capi.INVALID_ARGUMENT
    assert A.dropout_mha_ptr(0, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18, 0.5, 1, 2, 0) == 0, _capi.last_error()   # heads = 0
    assert A.dropout_mha_ptr(3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 0, O, 18, 0.5, 1, 2, 0) == 0, _capi.last_error()   # d = 0
    assert A.dropout_mha_ptr(3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18, 1.0, 1, 2, 0) == INV                     # p = 1
    assert A.dropout_mha_ptr(3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18, 0.5, 1, 2, -1) == INV                    # head0 < 0
    assert A.dropout_gat_ptr(3, 0.2, None, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18, float("nan"), 1, 2, 0) == INV
    assert A.dropout_mask_ptr(0, 0.5, 1, 2, 0, None, 0) == 0
    torch.cuda.synchronize()
    assert bool((O == POISON).all())
    # k = 0: every score the bias alone; dQ has no element
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))
    got = _drop(A, mat, Q0, K0, V, dO, 0.5, Bt=Bt, scale=0.7)
    keep, cd = DR.mask(mat.nnz, 3, 0.5, SEED, OFFSET), DR.cd_of(0.5, dtype)
    zq, zk = np.zeros((mat.m, 3, 0), dtype=dtype), np.zeros((mat.n, 3, 0), dtype=dtype)
    rho, want, allow = DR.allowances(mat, 0.7, _np(Bt), zq, zk, _np(V), _np(dO), keep, cd, dtype, STAGES)
    for i in (0, 3, 4):
        assert DR.compare(_np(got[i]), want[i], allow[i], NAMES[i]) <= 1.0, NAMES[i]
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0 with m > 0: +0 everywhere, no element of dB, no byte of the mask
    A = _open(none, np.zeros(0), dtype)
    Q, K, V, dO = _operands(none, 3, 4, 6, dtype, seed=3743)
    for t in _drop(A, none, Q, K, V, dO, 0.5, Bt=torch.zeros((0, 3), dtype=_tdt(dtype), device=DEV), scale=2.0):
        assert not _bits(_np(t)).any()
    for t in _gat(A, none, Q, K, V, dO, None, 0.2, None, 2.0, drop=(0.5, 1, 2, 0)):
        assert not _bits(_np(t)).any()
    assert A.dropoutMask(torch.zeros((0, 3), dtype=torch.uint8, device=DEV), 0.5, 1) == 0
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_calls_are_captured_on_their_first_use_and_a_replay_repeats_the_mask(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    Bt = _dev(EB.distinct_bias(mat, 3, 3760), dtype)
    a = _dev(np.random.default_rng(3761).uniform(-1, 1, size=(3, 5)), dtype)
    Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=3762)
    shapes = ((mat.m, 3, 6), tuple(Q.shape), tuple(K.shape), tuple(V.shape), (mat.nnz, 3))
    outs = [torch.full(s, POISON, dtype=_tdt(dtype), device=DEV) for s in shapes]
    gouts = [torch.full(s, POISON, dtype=_tdt(dtype), device=DEV) for s in shapes + (tuple(Q.shape),)]
    work, gwork = _work(mat, Q), _work(mat, Q)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.dropoutMha(Q, K, V, outs[0], 0.6, SEED, OFFSET, B=Bt, scale=0.4) == 0, _capi.last_error()
        assert A.dropoutMhaBackward(Q, K, V, dO, 0.6, SEED, OFFSET, dQ=outs[1], dK=outs[2], dV=outs[3], work=work, B=Bt, scale=0.4,
                                    dB=outs[4]) == 0, _capi.last_error()
        assert A.dropoutGat(Q, K, V, gouts[0], 0.6, SEED, OFFSET, a=a, B=Bt, scale=0.4) == 0, _capi.last_error()
        assert A.dropoutGatBackward(Q, K, V, dO, 0.6, SEED, OFFSET, dQ=gouts[1], dK=gouts[2], dV=gouts[3], work=gwork, a=a, B=Bt, scale=0.4,
                                    dB=gouts[4], dAr=gouts[5]) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    Bt.copy_(_dev(EB.distinct_bias(mat, 3, 3763), dtype))  # changed in place: the graph reads the same addresses
    replays = []
    for _ in range(2):
        for t in outs + gouts:
            t.fill_(POISON)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in outs + gouts])
    del graph
    assert A.setStream(None) == 0
    eager = _drop(A, mat, Q, K, V, dO, 0.6, Bt=Bt, scale=0.4) + _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.4, drop=(0.6, SEED, OFFSET, 0))
    for r in replays:
        for g, e, n in zip(r, eager, NAMES + GNAMES):
            assert _same(g, e), n
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("history", ("loaded", "reconverted"))
def test_a_loaded_and_a_reconverted_handle_give_the_fresh_handles_bits(history, dtype, tmp_path):
    mat = _zoo()["class-edges"]
    val = HH.values(mat, 3780, dtype)
    fresh = _open(mat, val, dtype, 7)
    old, _ = (HH._loaded if history == "loaded" else HH._reconverted)(mat, val, dtype, tmp_path)
    Q, K, V, dO = _operands(mat, 3, 3, 5, dtype, seed=3781)
    Bt = _dev(EB.distinct_bias(mat, 3, 3782), dtype)
    a = _dev(np.random.default_rng(3783).uniform(-1, 1, size=(3, 3)), dtype)
    res = []
    for A in (fresh, old):
        if not A.info().transpose_built:
            assert A.buildTranspose() == 0, _capi.last_error()
        res.append(_drop(A, mat, Q, K, V, dO, 0.6, Bt=Bt, scale=0.3) + _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(0.1, 5, 6, 1)))
    for g, w, n in zip(res[1], res[0], NAMES + GNAMES):
        assert not bool(torch.isnan(g).any()) and _same(g, w), (history, n)
    _close(fresh)
    _close(old)


# ---- 8. autograd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_autograd_evaluation_training_and_nothing_to_do(dtype):
    mat = EB.random_matrix()
    heads, k, d = 3, 8, 16
    A = _open(mat, np.random.default_rng(3800).uniform(-1, 1, size=mat.nnz), dtype)
    stored = A._arrays[2].clone()
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, 3801)
    Bt = _dev(EB.distinct_bias(mat, heads, 3802), dtype)
    a = _dev(np.random.default_rng(3803).uniform(-1, 1, size=(heads, k)), dtype)
    # evaluation: bit for bit the undropped functions
    with torch.no_grad():
        assert _same(autograd.dropout_attention(A, Q, K, V, 0.6, 9, scale=0.3, bias=Bt, training=False),
                     autograd.multihead_attention(A, Q, K, V, scale=0.3, bias=Bt))
        assert _same(autograd.dropout_attention(A, Q, K, V, 0.6, 9, training=False), autograd.multihead_attention(A, Q, K, V))
        assert _same(autograd.gat_dropout_attention(A, Q, K, V, 0.6, 9, att=a, scale=0.3, bias=Bt, training=False),
                     autograd.gat_attention(A, Q, K, V, att=a, scale=0.3, bias=Bt))
        assert _same(autograd.dropout_attention(A, Q, K, V, 0.0, 9, scale=0.3, bias=Bt), autograd.multihead_attention(A, Q, K, V, scale=0.3, bias=Bt))
    # training: the direct calls' words, in the output and in every gradient; a fixed seed makes the function deterministic
    q, k_, v, b = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
    out = autograd.dropout_attention(A, q, k_, v, 0.6, SEED, offset=OFFSET, scale=0.3, bias=b)
    out.backward(dO)
    torch.cuda.synchronize()
    for g, w, n in zip((out.detach(), q.grad, k_.grad, v.grad, b.grad), _drop(A, mat, Q, K, V, dO, 0.6, Bt=Bt, scale=0.3), NAMES):
        assert _same(g, w), n
    with torch.no_grad():
        assert _same(autograd.dropout_attention(A, Q, K, V, 0.6, SEED, offset=OFFSET, scale=0.3, bias=Bt), out.detach())
        assert not _same(autograd.dropout_attention(A, Q, K, V, 0.6, SEED, offset=OFFSET + 1, scale=0.3, bias=Bt), out.detach())
    q, k_, v, b, att = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt, a))
    out = autograd.gat_dropout_attention(A, q, k_, v, 0.1, SEED, offset=OFFSET, att=att, negative_slope=0.2, scale=0.3, bias=b)
    out.backward(dO)
    torch.cuda.synchronize()
    direct = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3, drop=(0.1, SEED, OFFSET, 0))
    for g, w, n in zip((out.detach(), q.grad, k_.grad, v.grad, b.grad), direct[:5], NAMES):
        assert _same(g, w), ("gat", n)
    assert _same(att.grad, direct[5].sum(0))
    assert _same(A._arrays[2], stored)                                         # the handle's values are untouched
    # nothing needs a gradient: nothing runs in backward
    calls = []
    real, greal = A.dropoutMhaBackward, A.dropoutGatBackward
    A.dropoutMhaBackward = lambda *ar, **kw: calls.append(1) or real(*ar, **kw)
    A.dropoutGatBackward = lambda *ar, **kw: calls.append(1) or greal(*ar, **kw)
    assert not autograd.dropout_attention(A, Q, K, V, 0.6, 1).requires_grad
    other = torch.ones((), dtype=_tdt(dtype), device=DEV, requires_grad=True)
    (autograd.dropout_attention(A, Q, K, V, 0.6, 1).sum() * other).backward()
    (autograd.gat_dropout_attention(A, Q, K, V, 0.6, 1, att=a).sum() * other).backward()
    torch.cuda.synchronize()
    assert calls == []
    del A.dropoutMhaBackward, A.dropoutGatBackward
    _close(A)


def test_gradcheck_with_a_fixed_seed():
    """fp64 on kat0: a fixed (seed, offset) makes both functions deterministic, differentiable functions of their inputs"""
    mat = _zoo()["kat0"]
    A = _open(mat, np.ones(mat.nnz), np.float64)
    rng = np.random.default_rng(3900)
    heads, k, d = 2, 3, 2
    Q, K, V = (_uniform(rng, s, np.float64).requires_grad_(True) for s in ((mat.m, heads, k), (mat.n, heads, k), (mat.n, heads, d)))
    Bt = _uniform(rng, (mat.nnz, heads), np.float64).requires_grad_(True)
    a = _uniform(rng, (heads, k), np.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q, k_, v, b: autograd.dropout_attention(A, q.clone(), k_.clone(), v.clone(), 0.5, 11, offset=3,
                                                                                    scale=0.7, bias=b.clone()), (Q, K, V, Bt))
    # (the LeakyReLU's kink: u = q + k stays away from 0 by more than gradcheck's step for these draws with probability one)
    assert torch.autograd.gradcheck(lambda q, k_, v, b, at: autograd.gat_dropout_attention(A, q.clone(), k_.clone(), v.clone(), 0.5, 11,
                                                                                            offset=3, att=at.clone(), scale=0.7,
                                                                                            bias=b.clone()), (Q, K, V, Bt, a))
    _close(A)
