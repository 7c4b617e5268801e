"""csr5hip_gat / csr5hip_gat_backward (``A.gat``, ``A.gatBackward``) and ``autograd.gat_attention`` on the GPU: additive attention,
softmax(scale sum_c a_c LeakyReLU(q_c + k_c) + B) on the pattern.  Tests 1, 2, 4 and 6 are identities that hold bit for bit; 3 is a
per-line bound on the accumulations against the call's own ds; 5 and 7 go to a float64 torch reference under the allowance of
tests/gat_reference.py.

WHY THE IDENTITIES HOLD.  (1) tests/gat_reference.py ``scores`` restates the score chain in numpy, bit for bit, for a in
{1, 1/2, -1, 2} and a scale that is a power of two.  The edge call with k = 0 computes s = fma(+0, 1, B') = B', so with B' those
scores it runs EXISTING code -- softmax, product, dV, dB -- on the same scores: O, dV and dB must be equal bits.  (2) fma(1, l, z)
has the bits of z + l, which is what a = None computes; head h of a packed call is the H = 1 call on the slices (csr5hip_mha's
contract).  (3) dQ, dK and dAr are sums over a line of t_e w_ec resp. t_e l_ec with t_e = ds_e c; ds_e is the dB the call writes,
shown by (1) to be existing code's.  The sum in extended precision on the CPU and the kernel's differ by at most gamma(L + 2) times
the sum of the absolute terms: L - 1 additions and the roundings of t and of w (or l: u is formed in the handle's type exactly as
the kernel forms it, so ns u is its one rounding).  One entry lost or counted twice in a line of 4 097 is far outside that.
(4) on a pattern of 16 entries per row with k = 2, a = (1, -1), K[j] = (x_j, x_j), Q = +0: l = (l_j, l_j), z = fma(-1, l_j, l_j)
= +0, every score +0 and p = 1/16, while g and l differ from entry to entry; dQ, dK and dAr are integers over 512 and dV over 16
in every order.

THE HEAD GROUPS are the rule's (att_heads_per_group), a function of the line count: on class-edges, class-edges^T and dealt 3 heads
are groups of two and one and 8 heads four groups of two; 8 heads are groups of 3 + 3 + 2 at 90 113 lines and ONE group at
262 145, on ``many_lines`` as in tests/test_gpu_attention_edges.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import autograd  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import edge_bias_reference as EB  # noqa: E402
from tests import gat_reference as G  # noqa: E402
from tests import handle_history as HH  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.exact_reference import unit_roundoff  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index, _uniform, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _bits, _close, _handle  # noqa: E402
from tests.test_gpu_mha_bias import _mask  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
POISON = -777.25
NAMES = G.NAMES
SHAPES = ((1, 1, 16), (3, 1, 5), (3, 3, 5), (2, 13, 70))
SLOPES = (0.2, 0.0, 1.0)


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
    return _handle(mat, np.asarray(val, dtype=dtype), Path("gat", sigma, H.SPMV_FUSED), dtype)[0]


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


def _gat(A, mat, Q, K, V, dO, a=None, ns=0.2, Bt=None, scale=1.0):
    """[O, dQ, dK, dV, dB, dAr] of gat / gatBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dB, dAr = _nan((mat.nnz, Q.shape[1]), Q), _nan(Q.shape, Q)
    assert A.gat(Q, K, V, O, a=a, negative_slope=ns, B=Bt, scale=scale) == 0, _capi.last_error()
    assert A.gatBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q), a=a, negative_slope=ns, B=Bt, scale=scale, dB=dB,
                         dAr=dAr) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dB, dAr]


def _yardstick(A, mat, Bp, V, dO):
    """[O, dV, dB] of the edge call with k = 0, null Q and K and B = B': existing code on given scores"""
    heads, d = V.shape[1], V.shape[2]
    O, dV, dB = _nan((mat.m, heads, d), V), _nan(V.shape, V), _nan(Bp.shape, Bp)
    work = torch.empty(4 * mat.m * heads, dtype=V.dtype, device=DEV)
    assert A.mha_edge_bias_ptr(heads, 1.0, Bp, heads, None, 0, None, 0, 0, V, heads * d, d, O, heads * d) == 0, _capi.last_error()
    assert A.mha_edge_bias_backward_ptr(heads, 1.0, Bp, heads, None, 0, None, 0, 0, V, heads * d, d, dO, heads * d, None, 0, None, 0, dV,
                                        heads * d, work, dB, heads) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O, dV, dB]


def _same(a, b):
    return E.same_bits(a.cpu().numpy(), b.cpu().numpy())


def _written(ts, what):
    for t, n in zip(ts, NAMES):
        assert not bool(torch.isnan(t).any()), (what, n, "an element was not written")


def _np(t):
    return t.cpu().numpy()


# ---- 1. the score through existing code ---------------------------------------------------------------------------------------------
def _score_case(A, mat, heads, k, d, dtype, seed, a_given, ns, with_b):
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed)
    an = G.exact_a(heads, k, dtype) if a_given else None
    bn = EB.distinct_bias(mat, heads, seed + 1).astype(dtype) if with_b else None
    scale = 0.25 if with_b else 1.0
    s = G.scores(mat, _np(Q), _np(K), an, ns, scale, bn, dtype)
    got = _gat(A, mat, Q, K, V, dO, a=_dev(an, dtype) if a_given else None, ns=ns, Bt=_dev(bn, dtype) if with_b else None, scale=scale)
    what = (mat.name, _dt(dtype), heads, k, d, "a" if a_given else "a=None", ns, "B, 1/4" if with_b else "no B")
    _written(got, what)
    want = _yardstick(A, mat, _dev(s, dtype), V, dO)
    for g, w, n in zip((got[0], got[3], got[4]), want, ("O", "dV", "dB")):
        assert _same(g, w), what + (n,)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("half-empty", "aligned64", "aligned1024", "two-hubs", "duplicates", "class-edges", "class-edges^T", "dealt"))
def test_the_score_has_the_bits_of_the_chain_restated_in_numpy(name, dtype):
    """O, dV and dB against the edge call with k = 0 on the numpy scores: every shape with a = None and a given, every slope, with
    and without (B, scale 1/4) -- the full cross"""
    mat = _zoo()[name]
    A = _open(mat, np.full(mat.nnz, 3.5), dtype)  # (values that would show in every score if they were read)
    assert A.buildTranspose() == 0, _capi.last_error()
    for si, (heads, k, d) in enumerate(SHAPES):
        for a_given in (False, True):
            for ns in SLOPES:
                for with_b in (False, True):
                    _score_case(A, mat, heads, k, d, dtype, 2100 + si, a_given, ns, with_b)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("heads", (3, 8))
@pytest.mark.parametrize("name", ("class-edges", "class-edges^T", "dealt"))
def test_the_score_chain_in_every_head_group_of_the_class_matrices(name, heads, dtype):
    """3 heads: groups of two and one; 8 heads: four groups of two (the rule at these line counts)"""
    mat = _zoo()[name]
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    _score_case(A, mat, heads, 3, 5, dtype, 2200 + heads, True, 0.2, True)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("lines,per_group", ((90113, 3), (262145, 8)), ids=("3+3+2", "one-group"))
def test_the_score_chain_with_eight_heads_in_wide_groups(lines, per_group, dtype):
    assert E.heads_per_group(lines, 8) == per_group
    mat = E.many_lines(lines)
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    _score_case(A, mat, 8, 3, 5, dtype, 2250, True, 0.2, True)
    _close(A)


# ---- 2. a = None is a = 1, and a head is the single-head call -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("half-empty", "two-hubs", "class-edges", "class-edges^T", "dealt"))
def test_null_a_is_ones_and_every_head_is_the_single_head_call(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    for si, (heads, k, d) in enumerate(((3, 1, 5), (3, 3, 5))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, 2300 + si)
        Bt = _dev(EB.distinct_bias(mat, heads, 2310 + si), dtype)
        ones = torch.ones((heads, k), dtype=Q.dtype, device=DEV)
        with_none, with_ones = _gat(A, mat, Q, K, V, dO, None, 0.2, Bt, 0.3), _gat(A, mat, Q, K, V, dO, ones, 0.2, Bt, 0.3)
        _written(with_none, name)
        for g, w, n in zip(with_none, with_ones, NAMES):
            assert _same(g, w), (name, heads, k, d, n, "a = None against ones")
        a = _dev(np.random.default_rng(2320 + si).uniform(-1, 1, size=(heads, k)), dtype)
        packed = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3)
        for h in range(heads):
            sl = slice(h, h + 1)
            one = _gat(A, mat, Q[:, sl], K[:, sl], V[:, sl], dO[:, sl], a[sl], 0.2, Bt[:, sl], 0.3)
            for g, w, n in zip(packed, one, NAMES):
                assert _same(g[:, sl].contiguous(), w), (name, heads, k, d, n, "head", h)
    _close(A)


# ---- 3. dQ, dK and dAr against the call's own ds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("two-hubs", "class-edges", "class-edges^T", "dealt"))
def test_the_accumulations_against_the_calls_own_ds(name, dtype):
    """|got - ref| <= gamma(L + 2) sum |t_e| |w_ec| per element (dAr: |l_ec|), L the line's length: the module docstring's (3)"""
    mat = _zoo()[name]
    rows, cols = G.rows_cols(mat)
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    u = unit_roundoff(dtype)
    ld = np.longdouble
    for si, (heads, k, d, a_given) in enumerate(((3, 3, 5, True), (3, 1, 5, False))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, 2400 + si)
        an = np.random.default_rng(2410 + si).uniform(-1, 1, size=(heads, k)).astype(dtype) if a_given else None
        Bt = _dev(EB.distinct_bias(mat, heads, 2420 + si), dtype)
        ns, c = dtype(0.2), dtype(0.3)
        got = [_np(t) for t in _gat(A, mat, Q, K, V, dO, _dev(an, dtype) if a_given else None, 0.2, Bt, 0.3)]
        uu = _np(Q)[rows] + _np(K)[cols]                                   # the handle's type: the kernel's u, its bits
        assert uu.dtype == np.dtype(dtype)
        t = got[4].astype(ld) * ld(c)                                      # t_e = ds_e c before its rounding
        g = np.where(uu > 0, ld(1), ld(ns))
        w = g if an is None else an.astype(ld)[None] * g
        l = np.where(uu > 0, uu.astype(ld), ld(ns) * uu.astype(ld))
        for what, gi, idx, lines, second in (("dQ", 1, rows, mat.m, w), ("dK", 2, cols, mat.n, w), ("dAr", 5, rows, mat.m, l)):
            ref, mag = np.zeros((lines, heads, k), dtype=ld), np.zeros((lines, heads, k), dtype=ld)
            np.add.at(ref, idx, t[:, :, None] * second)
            np.add.at(mag, idx, np.abs(t)[:, :, None] * np.abs(second))
            L = np.bincount(idx, minlength=lines).astype(np.float64) + 2
            gamma = (L * u / (1 - L * u))[:, None, None]
            err = np.abs(got[gi].astype(ld) - ref)
            assert (err <= gamma * mag).all(), (name, _dt(dtype), heads, k, what, float((err / np.maximum(gamma * mag, 1e-300)).max()))
    _close(A)


# ---- 4. order-independent exact expectations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_exact_backward_with_scores_of_zero_and_operands_that_differ(dtype):
    """the module docstring's (4) on ``dealt``: 16 entries in every row, columns of every class"""
    mat = _zoo()["dealt"]
    rows, cols = G.rows_cols(mat)
    heads, k, d = 2, 2, 5
    rng = np.random.default_rng([2500, 64 if dtype == np.float64 else 32])
    x = rng.integers(-2, 3, size=(mat.n, heads))
    Kn = np.repeat(x[:, :, None], k, axis=2).astype(dtype)
    Vn, dOn = rng.integers(-2, 3, size=(mat.n, heads, d)), rng.integers(-2, 3, size=(mat.m, heads, d))
    an = np.tile(np.array([1.0, -1.0], dtype=dtype), (heads, 1))
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q = torch.zeros((mat.m, heads, k), dtype=_tdt(dtype), device=DEV)
    got = [_np(t) for t in _gat(A, mat, Q, _dev(Kn, dtype), _dev(Vn, dtype), _dev(dOn, dtype), _dev(an, dtype), 0.5, None, 1.0)]
    _close(A)
    # in int64: 256 ds = 16 dp - 16 D; 2 g in {2, 1}; 2 l in {2 x, x}: dQ, dK and dAr in units of 1/512, dV of 1/16, O of 1/16
    dp = (dOn[rows] * Vn[cols]).sum(axis=2)                                                      # (nnz, H) integers
    D16 = np.zeros((mat.m, heads), dtype=np.int64)
    np.add.at(D16, rows, dp)
    ds256 = 16 * dp - D16[rows]
    xe = x[cols]                                                                                  # u = x_j in both channels
    g2 = np.where(xe > 0, 2, 1)
    l2 = np.where(xe > 0, 2 * xe, xe)
    sign = np.array([1, -1])
    w2 = g2[:, :, None] * sign[None, None, :]
    worst = 0

    def scatter(idx, n, terms):
        nonlocal worst
        out, mag = np.zeros((n,) + terms.shape[1:], dtype=np.int64), np.zeros((n,) + terms.shape[1:], dtype=np.int64)
        np.add.at(out, idx, terms)
        np.add.at(mag, idx, np.abs(terms))
        worst = max(worst, int(mag.max()))
        return out
    want = {"dQ": scatter(rows, mat.m, ds256[:, :, None] * w2).astype(dtype) / dtype(512),
            "dK": scatter(cols, mat.n, ds256[:, :, None] * w2).astype(dtype) / dtype(512),
            "dAr": scatter(rows, mat.m, ds256[:, :, None] * np.repeat(l2[:, :, None], k, axis=2)).astype(dtype) / dtype(512),
            "dV": scatter(cols, mat.n, dOn[rows]).astype(dtype) / dtype(16),
            "O": scatter(rows, mat.m, Vn[cols]).astype(dtype) / dtype(16),
            "dB": ds256.astype(dtype) / dtype(256)}
    worst = max(worst, int(np.abs(ds256).max()), int(np.bincount(rows, np.abs(dp).sum(axis=1)).max()))
    assert worst < E.EXACT_LIMIT, worst
    assert (g2 == 1).any() and (g2 == 2).any() and len(np.unique(l2)) >= 4  # (g and l differ from entry to entry)
    for n, g in zip(NAMES, got):
        assert E.same_bits(g, want[n] + dtype(0)), (n, _dt(dtype))  # (+ 0: an exact cancellation is +0, never -0)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_exact_forward_under_a_mask_of_minus_infinity(dtype):
    """Q = K = +0: z = +0 whatever a and ns, s = fma(+0, c, b) = b in {0, -Inf}: the mean of the unmasked rows of V"""
    mat = _zoo()["class-edges"]
    keep = _mask(mat, 600)
    mixed, dead = E.mask_conditions(mat, keep)
    assert mixed and 0 < dead < 0.5
    heads, k, d = 2, 3, 5
    rng = np.random.default_rng(2550)
    keeps = [keep, np.ones(mat.nnz, dtype=bool)]
    Vn = rng.integers(-1000, 1001, size=(mat.n, heads, d)).astype(dtype)
    Q, K = (torch.zeros((r, heads, k), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))
    Bt = _dev(np.stack([np.where(kh, 0.0, -np.inf) for kh in keeps], axis=1), dtype)
    a = _dev(np.random.default_rng(2551).uniform(-1, 1, size=(heads, k)), dtype)
    A = _open(mat, np.ones(mat.nnz), dtype)
    O = _nan((mat.m, heads, d), Q)
    assert A.gat(Q, K, _dev(Vn, dtype), O, a=a, negative_slope=0.2, B=Bt, scale=0.5) == 0, _capi.last_error()
    torch.cuda.synchronize()
    _close(A)
    for h in range(heads):
        want, mag = E.exact_forward(mat, Vn[:, h], keeps[h], dtype)
        assert mag < E.EXACT_LIMIT
        assert E.same_bits(_np(O)[:, h], want), h


# ---- 5. the float64 reference ---------------------------------------------------------------------------------------------------------
def _case_f(mat, dtype, seed, heads=G.F_HEADS, k=G.F_K, d=G.F_D):
    a, ns, bias, c, ops = G.case(mat, heads, k, d, dtype, seed)
    return _dev(a, dtype), ns, _dev(bias, dtype), c, tuple(_dev(t, dtype) for t in ops)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("which", ("class-edges", "random"))
def test_gat_calls_match_the_float64_reference(which, dtype):
    mat = _zoo()["class-edges"] if which == "class-edges" else G.random_matrix()
    rows, cols = _index(mat)
    a, ns, Bt, c, (Q, K, V, dO) = _case_f(mat, dtype, G.F_SEEDS[which])
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    got = _gat(A, mat, Q, K, V, dO, a, G.F_SLOPE, Bt, 1 / np.sqrt(G.F_K))
    _close(A)
    want = G.reference(mat, rows, cols, c, a, ns, Bt, Q, K, V, dO)
    allow = G.allowances(mat, rows, cols, c, a, ns, Bt, Q, K, V, dO, dtype, STAGES)
    print(f"{mat.name} {_dt(dtype)}: rho {allow[0]:.3e}")
    assert STAGES * allow[0] <= FIRST_ORDER, (mat.name, allow[0])
    for g, w, al, what in zip(got, want, allow[1:], NAMES):
        _within(g, w, al, f"{mat.name} {_dt(dtype)} {what}")


# ---- 6. the remaining guarantees ------------------------------------------------------------------------------------------------------
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
def test_guarded_writes_nan_values_and_nan_padding(dtype):
    """poison beyond every leading dimension; NaN in the handle's values (the companion's too) and in the padding of B"""
    heads, k, d = 3, 3, 5
    for name in ("half-empty", "aligned1024", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, np.ones(mat.nnz), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        nans = torch.full((mat.nnz,), float("nan"), dtype=_tdt(dtype), device=DEV)
        assert A.updateValues(nans) == 0, _capi.last_error()  # (the companion holds NaN too: updateValues keeps it current)
        torch.cuda.synchronize()
        Bt = _dev(EB.distinct_bias(mat, heads, 2600), dtype)
        wide = torch.full((mat.nnz, heads + 3), float("nan"), dtype=_tdt(dtype), device=DEV)
        wide[:, :heads] = Bt
        Bv = wide[:, :heads]
        a = _dev(np.random.default_rng(2601).uniform(-1, 1, size=(heads, k)), dtype)
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=2602)
        keep = [t.clone() for t in (Q, K, V, dO, wide, a)]
        info0 = bytes(A.info())
        want = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3)
        _written(want, name)
        shapes = ((mat.m, d), (mat.m, k), (mat.n, k), (mat.n, d))
        bufs = [_guarded(r, heads * w, dtype) for r, w in shapes] + [_guarded(mat.nnz, heads, dtype), _guarded(mat.m, heads * k, dtype)]
        views = [b[1].unflatten(1, (heads, w)) for b, (_, w) in zip(bufs[:4], shapes)] + [bufs[4][1], bufs[5][1].unflatten(1, (heads, k))]
        assert A.gat(Q, K, V, views[0], a=a, negative_slope=0.2, B=Bv, scale=0.3) == 0, _capi.last_error()
        assert A.gatBackward(Q, K, V, dO, views[1], views[2], views[3], _work(mat, Q), a=a, negative_slope=0.2, B=Bv, scale=0.3,
                             dB=views[4], dAr=views[5]) == 0, _capi.last_error()
        torch.cuda.synchronize()
        assert bytes(A.info()) == info0
        widths = (heads * d, heads * k, heads * k, heads * d, heads, heads * k)
        for (b, _, ld), w, width, rws, what in zip(bufs, want, widths, (mat.m, mat.m, mat.n, mat.n, mat.nnz, mat.m), NAMES):
            body = _guard_intact(b, rws, width, ld)
            assert np.array_equal(_bits(body), _bits(w.reshape(rws, -1).cpu().numpy())), (name, what)
        for t, k0 in zip((Q, K, V, dO, wide, a), keep):
            assert _same(t, k0)  # the operands are only read
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_each_output_alone_and_the_row_side_without_a_companion(dtype):
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, np.ones(mat.nnz), dtype)
        heads, k, d = 3, 3, 5
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=2620)
        Bt = _dev(EB.distinct_bias(mat, heads, 2621), dtype)
        a = _dev(np.random.default_rng(2622).uniform(-1, 1, size=(heads, k)), dtype)
        kw = dict(a=a, negative_slope=0.2, B=Bt, scale=0.7)
        # dK without a companion: INVALID_ARGUMENT and a text with the call's own name; dQ, dAr and dB need neither it nor work
        assert A.gatBackward(Q, K, V, dO, dK=torch.empty_like(K), work=_work(mat, Q), **kw) == _capi.INVALID_ARGUMENT
        assert "transposed companion" in _capi.last_error() and "csr5hip_gat_backward" in _capi.last_error()
        dQ, dAr, dB = _nan(Q.shape, Q), _nan(Q.shape, Q), _nan(Bt.shape, Bt)
        assert A.gatBackward(Q, K, V, dO, dQ=dQ, dB=dB, dAr=dAr, **kw) == 0, _capi.last_error()
        torch.cuda.synchronize()
        assert A.info().transpose_built == 0
        assert A.buildTranspose() == 0, _capi.last_error()
        full = _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.7)
        assert _same(dQ, full[1]) and _same(dB, full[4]) and _same(dAr, full[5])
        for i, key in ((1, "dQ"), (2, "dK"), (3, "dV"), (4, "dB"), (5, "dAr")):
            out = _nan(full[i].shape, Q)
            work = _work(mat, Q) if key in ("dK", "dV") else None
            assert A.gatBackward(Q, K, V, dO, work=work, **{key: out}, **kw) == 0, _capi.last_error()
            torch.cuda.synchronize()
            assert _same(out, full[i]), (name, key, "alone")
        assert A.gatBackward(Q, K, V, dO, **kw) == 0  # nothing wanted: a successful no-op
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_degenerate_shapes(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, 3, 4, 6, dtype, seed=2640)
    Bt = _dev(EB.distinct_bias(mat, 3, 2641), dtype)
    a = _dev(np.random.default_rng(2642).uniform(-1, 1, size=(3, 4)), dtype)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    dAr = torch.full((mat.m, 3, 4), POISON, dtype=_tdt(dtype), device=DEV)
    INV = _capi.INVALID_ARGUMENT
    assert A.gat_ptr(0, 0.2, a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == 0, _capi.last_error()  # heads = 0
    assert A.gat_ptr(3, 0.2, a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 0, O, 18) == 0, _capi.last_error()  # d = 0
    assert A.gat_backward_ptr(0, 0.2, a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, None, 3, dAr, 12) == 0
    assert A.gat_ptr(3, float("nan"), a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.gat_backward_ptr(3, float("inf"), a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, None, 3,
                              dAr, 12) == INV
    assert A.gat_backward_ptr(3, 0.2, a, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, None, 3, dAr,
                              11) == INV
    torch.cuda.synchronize()
    assert bool((O == POISON).all()) and bool((dAr == POISON).all())
    # k = 0 is the edge call with k = 0: z = +0, every score the bias alone; dQ and dAr have no element
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))
    O0, dV0, dB0 = _nan(O.shape, O), _nan(V.shape, V), _nan(Bt.shape, Bt)
    assert A.gat(Q0, K0, V, O0, a=torch.zeros((3, 0), dtype=_tdt(dtype), device=DEV), B=Bt, scale=0.7) == 0, _capi.last_error()
    assert A.gatBackward(Q0, K0, V, dO, dV=dV0, work=_work(mat, Q), B=Bt, scale=0.7, dB=dB0, dAr=torch.empty_like(Q0)) == 0, _capi.last_error()
    edge = [_nan(O.shape, O), _nan(V.shape, V), _nan(Bt.shape, Bt)]
    assert A.mhaEdgeBias(Q0, K0, V, edge[0], B=Bt, scale=0.7) == 0, _capi.last_error()
    assert A.mhaEdgeBiasBackward(Q0, K0, V, dO, dV=edge[1], work=_work(mat, Q), B=Bt, scale=0.7, dB=edge[2]) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert _same(O0, edge[0]) and _same(dV0, edge[1]) and _same(dB0, edge[2])
    # d = 0 in the backward: dB is the score gradient of an empty product, +0 wherever p is finite; dQ and dAr likewise
    V0, dO0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.n, mat.m))
    dB, dQ, dAr = _nan(Bt.shape, Bt), _nan(Q.shape, Q), _nan(Q.shape, Q)
    assert A.gatBackward(Q, K, V0, dO0, dQ=dQ, a=a, B=Bt, dB=dB, dAr=dAr) == 0, _capi.last_error()
    torch.cuda.synchronize()
    for t in (dB, dQ, dAr):
        assert not (_np(t) != 0).any() and not np.isnan(_np(t)).any()
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0 with m > 0: +0 everywhere, no element of dB
    assert none.m > 0 and none.nnz == 0
    A = _open(none, np.zeros(0), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(none, 3, 4, 6, dtype, seed=2643)
    for t in _gat(A, none, Q, K, V, dO, a, 0.2, torch.zeros((0, 3), dtype=_tdt(dtype), device=DEV), 2.0):
        assert not _bits(t.cpu().numpy()).any()
    _close(A)
    nothing = type(none)(0, 5, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), "no-rows")  # m = 0
    A = _open(nothing, np.zeros(0), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    rng = np.random.default_rng(2644)
    K, V = _uniform(rng, (5, 3, 4), dtype), _uniform(rng, (5, 3, 6), dtype)
    Q, dO = (torch.zeros((0, 3, w), dtype=_tdt(dtype), device=DEV) for w in (4, 6))
    none_b = torch.zeros((0, 3), dtype=_tdt(dtype), device=DEV)
    assert A.gat(Q, K, V, torch.zeros_like(dO), a=a, negative_slope=0.2, B=none_b, scale=2.0) == 0, _capi.last_error()  # a no-op
    dK, dV = _nan(K.shape, K), _nan(V.shape, V)
    assert A.gatBackward(Q, K, V, dO, torch.zeros_like(Q), dK, dV, torch.zeros(0, dtype=_tdt(dtype), device=DEV), a=a, negative_slope=0.2,
                         B=none_b, scale=2.0, dB=torch.zeros_like(none_b), dAr=torch.zeros_like(Q)) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not _bits(_np(dK)).any() and not _bits(_np(dV)).any()  # no row attends to anything: every gradient of K and V is +0
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_both_calls_are_captured_on_their_first_use(dtype):
    """the first gat and the first gatBackward of the handle are the captured ones; replayed after a and B changed in place"""
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Bt = _dev(EB.distinct_bias(mat, 3, 2660), dtype)
    a = _dev(np.random.default_rng(2661).uniform(-1, 1, size=(3, 5)), dtype)
    Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=2662)
    outs = [torch.full(s, POISON, dtype=_tdt(dtype), device=DEV)
            for s in ((mat.m, 3, 6), tuple(Q.shape), tuple(K.shape), tuple(V.shape), (mat.nnz, 3), tuple(Q.shape))]
    work = torch.empty(12 * mat.m, dtype=Q.dtype, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert A.gat(Q, K, V, outs[0], a=a, negative_slope=0.2, B=Bt, scale=0.4) == 0, _capi.last_error()
        assert A.gatBackward(Q, K, V, dO, outs[1], outs[2], outs[3], work, a=a, negative_slope=0.2, B=Bt, scale=0.4, dB=outs[4],
                             dAr=outs[5]) == 0, _capi.last_error()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    Bt.copy_(_dev(EB.distinct_bias(mat, 3, 2663), dtype))  # changed in place: the graph reads the same addresses
    a.mul_(-0.5)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in outs]
    del graph
    assert A.setStream(None) == 0
    for g, e, n in zip(replayed, _gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.4), NAMES):
        assert _same(g, e), n
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("history", ("loaded", "reconverted"))
def test_a_loaded_and_a_reconverted_handle_give_the_fresh_handles_bits(history, dtype, tmp_path):
    mat = _zoo()["class-edges"]
    val = HH.values(mat, 2680, dtype)
    fresh = _open(mat, val, dtype, 7)
    old, _ = (HH._loaded if history == "loaded" else HH._reconverted)(mat, val, dtype, tmp_path)
    Q, K, V, dO = _operands(mat, 3, 3, 5, dtype, seed=2681)
    Bt = _dev(EB.distinct_bias(mat, 3, 2682), dtype)
    a = _dev(np.random.default_rng(2683).uniform(-1, 1, size=(3, 3)), dtype)
    res = []
    for A in (fresh, old):
        if not A.info().transpose_built:
            assert A.buildTranspose() == 0, _capi.last_error()
        res.append(_gat(A, mat, Q, K, V, dO, a, 0.2, Bt, 0.3))
    _written(res[1], history)
    for g, w, n in zip(res[1], res[0], NAMES):
        assert _same(g, w), (history, n)
    _close(fresh)
    _close(old)


# ---- 7. autograd --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_gat_attention_gradients_match_the_float64_reference(dtype):
    for which in ("random", "class-edges"):
        mat = _zoo()["class-edges"] if which == "class-edges" else G.random_matrix()
        rows, cols = _index(mat)
        a, ns, Bt, c, (Q, K, V, dO) = _case_f(mat, dtype, G.F_SEEDS[which] + 5)
        A = _open(mat, np.random.default_rng(2900).uniform(-1, 1, size=mat.nnz), dtype)
        stored = A._arrays[2].clone()
        q, k_, v, att, b = (t.clone().requires_grad_(True) for t in (Q, K, V, a, Bt))
        out = autograd.gat_attention(A, q, k_, v, att=att, negative_slope=G.F_SLOPE, scale=1 / np.sqrt(G.F_K), bias=b)
        out.backward(dO)
        torch.cuda.synchronize()
        assert _same(A._arrays[2], stored) and A.info().transpose_built == 1
        direct = _gat(A, mat, Q, K, V, dO, a, G.F_SLOPE, Bt, 1 / np.sqrt(G.F_K))
        for g, w in zip((out.detach(), q.grad, k_.grad, v.grad, b.grad), direct[:5]):
            assert _same(g, w)
        assert _same(att.grad, direct[5].sum(0))  # grad_att IS dAr.sum(0)
        want = G.reference(mat, rows, cols, c, a, ns, Bt, Q, K, V, dO)
        allow = G.allowances(mat, rows, cols, c, a, ns, Bt, Q, K, V, dO, dtype, STAGES)
        assert STAGES * allow[0] <= FIRST_ORDER
        for g, w, al, what in zip((out.detach(), q.grad, k_.grad, v.grad, b.grad), want[:5], allow[1:6], NAMES):
            _within(g, w, al, f"{mat.name} {_dt(dtype)} autograd {what}")
        _within(att.grad, want[6], allow[7], f"{mat.name} {_dt(dtype)} autograd att")
        _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_gat_attention_with_one_tensor_as_k_and_v_and_without_gradients(dtype):
    mat = G.random_matrix()
    rows, cols = _index(mat)
    heads, w = 3, 8
    a, ns, _, c, (Q, X, _, dO) = _case_f(mat, dtype, 2950, heads, w, w)
    A = _open(mat, np.ones(mat.nnz), dtype)
    x = X.clone().requires_grad_(True)
    q = Q.clone().requires_grad_(True)
    out = autograd.gat_attention(A, q, x, x, att=a, scale=c)  # GATv2: the transformed features are K and V
    out.backward(dO)
    torch.cuda.synchronize()
    assert A.info().transpose_built == 1
    direct = _gat(A, mat, Q, X, X.clone(), dO, a, 0.2, None, c)
    assert _same(out.detach(), direct[0]) and _same(q.grad, direct[1])
    assert _same(x.grad, direct[2] + direct[3])  # autograd adds the two gradients
    want = G.reference(mat, rows, cols, c, a, ns, None, Q, X, X, dO)
    allow = G.allowances(mat, rows, cols, c, a, ns, None, Q, X, X, dO, dtype, STAGES)
    assert STAGES * allow[0] <= FIRST_ORDER
    _within(x.grad, want[2] + want[3], allow[3] + allow[4] + unit_roundoff(dtype) * (want[2].abs() + want[3].abs()),
            f"{_dt(dtype)} K and V one tensor")
    _close(A)
    # only Q needs a gradient: no companion is built; nothing needs one: nothing runs in backward
    A = _open(mat, np.ones(mat.nnz), dtype)
    q = Q.clone().requires_grad_(True)
    autograd.gat_attention(A, q, X, X, att=a, scale=c).backward(dO)
    torch.cuda.synchronize()
    assert A.info().transpose_built == 0 and _same(q.grad, direct[1])
    calls = []
    real = A.gatBackward
    A.gatBackward = lambda *ar, **kw: calls.append(1) or real(*ar, **kw)
    assert not autograd.gat_attention(A, Q, X, X, att=a, scale=c).requires_grad
    other = torch.ones((), dtype=_tdt(dtype), device=DEV, requires_grad=True)
    (autograd.gat_attention(A, Q, X, X, att=a, scale=c).sum() * other).backward()
    torch.cuda.synchronize()
    assert calls == []
    del A.gatBackward
    _close(A)
