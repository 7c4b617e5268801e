"""csr5hip_mha_edge_bias / csr5hip_mha_edge_bias_backward (``A.mhaEdgeBias``, ``A.mhaEdgeBiasBackward``) and
``autograd.multihead_attention(..., bias=B2d)`` on the GPU: softmax(scale Q K^T + B) on the pattern, B a caller-owned (nnz, H)
tensor in CSR order; the handle's values take no part.  Tests 1 to 6 are identities that hold bit for bit; 7 and 10 go to a
float64 torch reference under the allowance of tests/edge_bias_reference.py.

WHY THE IDENTITIES HOLD.  s = fma(qk, c, b), and everything after the score is csr5hip_mha's.  (1) b = +0 or no B, c = 1:
s = qk + 0, the plain score (a -0 becomes +0: the same value, and a score enters the rest only through s - M), t = ds * 1 = ds.
(2) b = slopes[h] * a formed in torch with slopes in {2, 0.5, -1, 1} and integer a: the product is exact, so torch's rounded
multiplication and the biased kernel's give the same number, the sign of a zero included, and the two kernels differ in nothing
but where that number is read from.  (3) head h of the packed call has the bits of the single-head call on that head's slices
(csr5hip_mha's contract, kept by the biased call); the single-head biased call on a handle that was given B[:, h] as values
reads, per entry, exactly the number the edge call reads at (e, h).  (6) Q = +0: qk = +0 and s = fma(+0, c, b) = b; with b in
{0, -Inf} the weights are 1 and +0 and O is a mean of integer rows of V (tests/attention_edges.py ``exact_forward``)."""
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
from tests import mha_bias_reference as B  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests import zoo  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index, _uniform, _within  # noqa: E402
from tests.test_gpu_exact_reference import DEV, Path, _bits, _close, _handle  # noqa: E402

AUTO = H.ANONYMOUSLIB_AUTO_TUNED_SIGMA
POISON = -777.25
NAMES = ("O", "dQ", "dK", "dV", "dB")


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
    return _handle(mat, np.asarray(val, dtype=dtype), Path("edge-bias", sigma, H.SPMV_FUSED), dtype)[0]


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


def _plain(A, mat, Q, K, V, dO):
    """[O, dQ, dK, dV] of mha / mhaBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    assert A.mha(Q, K, V, O) == 0, _capi.last_error()
    assert A.mhaBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q)) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs


def _biased(A, mat, Q, K, V, dO, scale=1.0, slopes=None):
    """[O, dQ, dK, dV, dS] of mhaBiased / mhaBiasedBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dS = _nan((mat.nnz, Q.shape[1]), Q)
    assert A.mhaBiased(Q, K, V, O, scale=scale, slopes=slopes) == 0, _capi.last_error()
    assert A.mhaBiasedBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q), scale=scale, slopes=slopes, dS=dS) == 0, \
        _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dS]


def _edge(A, mat, Q, K, V, dO, Bt=None, scale=1.0):
    """[O, dQ, dK, dV, dB] of mhaEdgeBias / mhaEdgeBiasBackward"""
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dB = _nan((mat.nnz, Q.shape[1]), Q)
    assert A.mhaEdgeBias(Q, K, V, O, B=Bt, scale=scale) == 0, _capi.last_error()
    assert A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], _work(mat, Q), B=Bt, scale=scale, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return [O] + outs + [dB]


def _same(a, b):
    return E.same_bits(a.cpu().numpy(), b.cpu().numpy())


def _written(ts, what):
    for t, n in zip(ts, NAMES):
        assert not bool(torch.isnan(t).any()), (what, n, "an element was not written")


# ---- 1. a zero or a null bias is mha ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ("half-empty", "aligned64", "aligned1024", "two-hubs"))
def test_zero_and_null_bias_are_mha(name, dtype):
    mat = _zoo()[name]
    A = _open(mat, np.full(mat.nnz, 3.5), dtype)  # (values that would show in every score if they were read)
    assert A.buildTranspose() == 0, _capi.last_error()
    for si, (heads, k, d) in enumerate(((1, 8, 16), (3, 3, 5), (2, 13, 70))):
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=1300 + si)
        want = _plain(A, mat, Q, K, V, dO)
        zero = torch.zeros((mat.nnz, heads), dtype=Q.dtype, device=DEV)
        with_zero, with_none = _edge(A, mat, Q, K, V, dO, zero), _edge(A, mat, Q, K, V, dO, None)
        _written(with_zero, (name, heads, k, d))
        for g0, gn, w, what in zip(with_zero, with_none, want, NAMES[:4]):
            assert _same(g0, w), ("B = +0", name, heads, k, d, what)
            assert _same(gn, w), ("B = None", name, heads, k, d, what)
        assert _same(with_zero[4], with_none[4])
    _close(A)


# ---- 2. a rank-one bias is mhaBiased ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("sigma", (AUTO, 4), ids=("auto", "sigma4"))
@pytest.mark.parametrize("name", ("half-empty", "aligned1024", "two-hubs", "class-edges", "dealt", "duplicates"))
def test_rank_one_bias_has_the_bits_of_the_biased_call(name, sigma, dtype):
    mat = _zoo()[name]
    _, _, a = B.rank_one(mat, seed=17)
    slopes = np.array([2.0, 0.5, -1.0, 1.0])
    A = _open(mat, a, dtype, sigma)
    assert A.buildTranspose() == 0, _capi.last_error()
    sl, av = _dev(slopes, dtype), _dev(a, dtype)
    Bt = av[:, None] * sl[None, :]  # (exact products: torch's multiplication and the biased kernel's agree bit for bit)
    assert np.array_equal(Bt.cpu().numpy().astype(np.float64), a[:, None] * slopes[None, :])
    for k, d in ((8, 16), (12, 16)):
        Q, K, V, dO = _operands(mat, 4, k, d, dtype, seed=1400 + k)
        got = _edge(A, mat, Q, K, V, dO, Bt, scale=0.25)
        _written(got, (name, k, d))
        for g, w, what in zip(got, _biased(A, mat, Q, K, V, dO, scale=0.25, slopes=sl), NAMES):
            assert _same(g, w), (name, A.info().sigma, k, d, what)
    _close(A)


# ---- 3. a genuinely per-head bias ------------------------------------------------------------------------------------------------
def _head_by_head(A2, mat, Q, K, V, dO, Bt, scale):
    """[O, dQ, dK, dV, dB] head by head: updateValues(B[:, h]) and the single-head biased calls on the column slices"""
    res = [_nan(t.shape, t) for t in (dO, Q, K, V)] + [_nan(Bt.shape, Bt)]
    for h in range(Q.shape[1]):
        assert A2.updateValues(Bt[:, h].contiguous()) == 0, _capi.last_error()
        one = _biased(A2, mat, Q[:, h:h + 1], K[:, h:h + 1], V[:, h:h + 1], dO[:, h:h + 1], scale=scale)
        for r, o in zip(res[:4], one[:4]):
            r[:, h] = o[:, 0]
        res[4][:, h] = one[4][:, 0]
    return res


def _per_head_case(mat, heads, dtype, seed):
    Bt = _dev(EB.distinct_bias(mat, heads, seed), dtype)
    assert torch.unique(Bt).numel() == Bt.numel()  # (distinct in the handle's type too)
    A = _open(mat, np.random.default_rng(seed).uniform(-1, 1, size=mat.nnz), dtype)
    A2 = _open(mat, np.zeros(mat.nnz), dtype)
    assert A.buildTranspose() == 0 and A2.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, heads, 8, 16, dtype, seed=seed + 1)
    got = _edge(A, mat, Q, K, V, dO, Bt, scale=0.3)
    _written(got, (mat.name, heads))
    want = _head_by_head(A2, mat, Q, K, V, dO, Bt, 0.3)
    for g, w, what in zip(got, want, NAMES):
        for h in range(heads):
            assert _same(g[:, h], w[:, h]), (mat.name, heads, what, "head", h)
    _close(A)
    _close(A2)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("heads", (3, 8))
@pytest.mark.parametrize("name", ("duplicates", "class-edges", "class-edges^T", "dealt"))
def test_every_head_has_the_bits_of_the_single_head_call_with_its_column_as_values(name, heads, dtype):
    """H = 3: one head group of three or groups of two and one; H = 8 on these matrices: four groups of two"""
    _per_head_case(_zoo()[name], heads, dtype, seed=1500 + heads)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_eight_heads_in_groups_of_three_three_and_two(dtype):
    """102 401 lines are 401 workgroups: the rule gives three head groups, of 3, 3 and 2 heads, on the row and on the column side"""
    m = 256 * 400 + 1
    assert E.heads_per_group(m, 8) == 3
    _per_head_case(E.many_lines(m), 8, dtype, seed=1520)


# ---- 4. the handle's values are not read -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_the_handles_values_are_neither_read_nor_written(dtype):
    for name in ("half-empty", "class-edges"):
        mat = _zoo()[name]
        rng = np.random.default_rng([1600, mat.nnz])
        A = _open(mat, rng.uniform(-1, 1, size=mat.nnz), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        Bt = _dev(EB.distinct_bias(mat, 3, 1601), dtype)
        Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=1602)
        info0, stored = bytes(A.info()), A._arrays[2].clone()
        first = _edge(A, mat, Q, K, V, dO, Bt, scale=0.4)
        assert bytes(A.info()) == info0 and _same(A._arrays[2], stored)
        _written(first, name)
        nans = torch.full((mat.nnz,), float("nan"), dtype=_tdt(dtype), device=DEV)
        assert A.updateValues(nans) == 0, _capi.last_error()  # (the companion holds NaN too: updateValues keeps it current)
        torch.cuda.synchronize()
        info1 = bytes(A.info())
        again = _edge(A, mat, Q, K, V, dO, Bt, scale=0.4)
        assert bytes(A.info()) == info1
        for g, w, what in zip(again, first, NAMES):
            assert _same(g, w), (name, what)
        assert A.asCSR() == 0, _capi.last_error()  # hands back the values last given
        torch.cuda.synchronize()
        assert bool(torch.isnan(A._arrays[2]).all())
        _close(A)


# ---- 5. only what is declared is read and written ----------------------------------------------------------------------------------
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
def test_only_the_declared_elements_are_read_and_written(dtype):
    heads, k, d = 3, 3, 5
    for name in ("half-empty", "aligned1024", "class-edges"):
        mat = _zoo()[name]
        A = _open(mat, np.ones(mat.nnz), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        Bn = EB.distinct_bias(mat, heads, 1650)
        Bt = _dev(Bn, dtype)
        wide = torch.full((mat.nnz, heads + 3), float("nan"), dtype=_tdt(dtype), device=DEV)  # ldb = H + 3, NaN in the padding
        wide[:, :heads] = Bt
        Bv = wide[:, :heads]
        Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=1651)
        keep = [t.clone() for t in (Q, K, V, dO, wide)]
        want = _edge(A, mat, Q, K, V, dO, Bt, scale=0.3)
        _written(want, name)
        bufs = [_guarded(r, heads * w, dtype) for r, w in ((mat.m, d), (mat.m, k), (mat.n, k), (mat.n, d))] + [_guarded(mat.nnz, heads, dtype)]
        views = [b[1].unflatten(1, (heads, w)) for b, w in zip(bufs[:4], (d, k, k, d))] + [bufs[4][1]]
        assert A.mhaEdgeBias(Q, K, V, views[0], B=Bv, scale=0.3) == 0, _capi.last_error()
        assert A.mhaEdgeBiasBackward(Q, K, V, dO, views[1], views[2], views[3], _work(mat, Q), B=Bv, scale=0.3, dB=views[4]) == 0, \
            _capi.last_error()
        torch.cuda.synchronize()
        for (b, _, ld), w, width, rws, what in zip(bufs, want, (heads * d, heads * k, heads * k, heads * d, heads),
                                                   (mat.m, mat.m, mat.n, mat.n, mat.nnz), NAMES):
            body = _guard_intact(b, rws, width, ld)  # (dB: its padding columns are untouched)
            assert np.array_equal(_bits(body), _bits(w.reshape(rws, -1).cpu().numpy())), (name, what)
        for t, k0 in zip((Q, K, V, dO), keep):
            assert torch.equal(t, k0)
        assert _same(wide, keep[4])  # B is only read
        # nothing wanted: a successful no-op, with or without operands
        assert A.mhaEdgeBiasBackward(Q, K, V, dO, B=Bv, scale=0.3) == 0, _capi.last_error()
        assert A.mha_edge_bias_backward_ptr(heads, 0.3, None, 0, None, 9, None, 9, k, None, 15, d, None, 15, None, 9, None, 9, None, 15, None,
                                            None, 3) == 0, _capi.last_error()
        _close(A)


# ---- 6. -Inf as a per-head mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_minus_infinity_masks_one_head_only(dtype):
    """head 0: one chosen entry of every row of two or more entries is masked, and every fifth non-empty row entirely; head 1:
    nothing is masked.  Q = +0, so every unmasked score is +0 and O is the mean of the unmasked rows of V."""
    mat = _zoo()["class-edges"]
    rng = np.random.default_rng(1660)
    rows, cols = E.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    lens = np.diff(mat.row_ptr)
    keep0 = np.ones(mat.nnz, dtype=bool)
    dead_rows = np.zeros(mat.m, dtype=bool)
    for n, i in enumerate(np.flatnonzero(lens > 0)):
        a, L = int(mat.row_ptr[i]), int(lens[i])
        if n % 5 == 4:
            keep0[a:a + L] = False
            dead_rows[i] = True
        elif L >= 2:
            keep0[a + int(rng.integers(L))] = False
    assert dead_rows.any() and (lens[dead_rows] > E.AT_G).any() and (lens[~dead_rows] > 2048).any()
    keep = [keep0, np.ones(mat.nnz, dtype=bool)]
    heads, k, d = 2, 3, 5
    Q = torch.zeros((mat.m, heads, k), dtype=_tdt(dtype), device=DEV)  # qk = +0: the score is the bias
    K = _uniform(rng, (mat.n, heads, k), dtype)
    Vn = rng.integers(-1000, 1001, size=(mat.n, heads, d)).astype(dtype)
    dOn = rng.integers(-8, 9, size=(mat.m, heads, d)).astype(dtype)
    V, dO = _dev(Vn, dtype), _dev(dOn, dtype)
    Bt = _dev(np.stack([np.where(kh, 0.0, -np.inf) for kh in keep], axis=1), dtype)
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    O, dQ, dK, dV, dB = (t.cpu().numpy() for t in _edge(A, mat, Q, K, V, dO, Bt, scale=0.5))
    _close(A)
    for h in range(heads):
        want, mag = E.exact_forward(mat, Vn[:, h], keep[h], dtype)
        assert mag < E.EXACT_LIMIT
        assert E.same_bits(O[:, h], want), h  # the exact mean of the unmasked V rows; NaN where the whole row is masked
    # a row masked entirely in head 0 is NaN in that head's columns only
    for t in (O, dQ):
        assert np.array_equal(np.isnan(t[:, 0]).all(axis=1), dead_rows) and np.array_equal(np.isnan(t[:, 0]).any(axis=1), dead_rows)
        assert not np.isnan(t[:, 1]).any()
    assert np.array_equal(np.isnan(dB[:, 0]), dead_rows[rows]) and not np.isnan(dB[:, 1]).any()
    # the masked weight is exactly +0: ds = p (dp - D) is a zero there, and the entry adds nothing to dV
    live_masked = ~keep0 & ~dead_rows[rows]
    assert live_masked.any() and not (dB[live_masked, 0] != 0).any()
    poisoned = np.zeros(mat.n, dtype=bool)
    poisoned[cols[dead_rows[rows]]] = True
    assert np.array_equal(np.isnan(dV[:, 0]).any(axis=1), poisoned) and np.array_equal(np.isnan(dK[:, 0]).any(axis=1), poisoned)
    assert not np.isnan(dV[:, 1]).any() and not np.isnan(dK[:, 1]).any()
    # dV[j] = sum over the unmasked entries of column j of dO[i] / kept_i: dyadic where kept_i is a power of two; here compared
    # with the float64 sum under one unit roundoff per term of the type
    for h in range(heads):
        kept = np.bincount(rows[keep[h]], minlength=mat.m)
        live = keep[h] & (kept[rows] > 0)
        want = np.zeros((mat.n, d))
        np.add.at(want, cols[live], dOn[rows[live], h].astype(np.float64) / kept[rows[live]][:, None])
        mags = np.zeros((mat.n, d))
        np.add.at(mags, cols[live], np.abs(dOn[rows[live], h]).astype(np.float64) / kept[rows[live]][:, None])
        ok = ~np.isnan(dV[:, h]).any(axis=1)
        n_terms = np.bincount(cols, minlength=mat.n).max()
        assert (np.abs(dV[ok, h] - want[ok]) <= (n_terms + 2) * np.finfo(dtype).eps * mags[ok]).all(), h


# ---- 7. the float64 reference ------------------------------------------------------------------------------------------------------
def _case_f(mat, dtype, seed):
    bias, c, ops = EB.case(mat, EB.F_HEADS, EB.F_K, EB.F_D, dtype, seed)
    return _dev(bias, dtype), c, tuple(_dev(t, dtype) for t in ops)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("which", ("class-edges", "random"))
def test_edge_bias_calls_match_the_float64_reference(which, dtype):
    mat = _zoo()["class-edges"] if which == "class-edges" else EB.random_matrix()
    rows, cols = _index(mat)
    Bt, c, (Q, K, V, dO) = _case_f(mat, dtype, EB.F_SEEDS[which])
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    got = _edge(A, mat, Q, K, V, dO, Bt, scale=1 / np.sqrt(EB.F_K))
    _close(A)
    want = EB.reference(mat, rows, cols, c, Bt, Q, K, V, dO)
    allow = EB.allowances(mat, rows, cols, c, Bt, Q, K, V, dO, dtype, STAGES)
    print(f"{mat.name} {_dt(dtype)}: rho {allow[0]:.3e}")
    assert STAGES * allow[0] <= FIRST_ORDER, (mat.name, allow[0])
    for g, w, a, what in zip(got, want, allow[1:], NAMES):
        _within(g, w, a, f"{mat.name} {_dt(dtype)} {what}")


# ---- 8. degenerate shapes and the error order on a real handle ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_degenerate_shapes_and_the_error_order(dtype):
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    Q, K, V, dO = _operands(mat, 3, 4, 6, dtype, seed=1810)
    Bt = _dev(EB.distinct_bias(mat, 3, 1811), dtype)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    dB = torch.full((mat.nnz, 3), POISON, dtype=_tdt(dtype), device=DEV)
    INV = _capi.INVALID_ARGUMENT
    assert A.mha_edge_bias_ptr(0, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, O, 18) == 0, _capi.last_error()  # heads = 0
    assert A.mha_edge_bias_ptr(3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 0, O, 18) == 0, _capi.last_error()  # d = 0
    assert A.mha_edge_bias_backward_ptr(0, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, dB, 3) == 0
    torch.cuda.synchronize()
    assert bool((O == POISON).all()) and bool((dB == POISON).all())
    # the scale, ldb and lddb are rejected on a converted handle too (their place in the order: tests/test_mha_edge_bias_host.py)
    assert A.mha_edge_bias_ptr(3, float("nan"), Bt, 3, None, 0, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.mha_edge_bias_ptr(3, 1.0, Bt, 2, Q, 12, K, 12, 4, V, 18, 6, O, 18) == INV
    assert A.mha_edge_bias_backward_ptr(3, float("inf"), Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, K, 12, None, 18, None, dB, 3) == INV
    assert A.mha_edge_bias_backward_ptr(3, 1.0, Bt, 3, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, dB, 2) == INV
    assert A.mha_edge_bias_backward_ptr(3, 1.0, Bt, 2, Q, 12, K, 12, 4, V, 18, 6, dO, 18, None, 12, None, 12, None, 18, None, dB, 3) == INV
    torch.cuda.synchronize()
    assert bool((O == POISON).all()) and bool((dB == POISON).all())
    # dK without a companion: INVALID_ARGUMENT and a text; dQ and dB need neither the companion nor the workspace
    dK = torch.empty_like(K)
    assert A.mhaEdgeBiasBackward(Q, K, V, dO, dK=dK, work=torch.empty(12 * mat.m, dtype=Q.dtype, device=DEV), B=Bt) == INV
    assert "transposed companion" in _capi.last_error() and "csr5hip_mha_edge_bias_backward" in _capi.last_error()
    dQ = _nan(Q.shape, Q)
    dB = _nan(Bt.shape, Bt)
    assert A.mhaEdgeBiasBackward(Q, K, V, dO, dQ=dQ, B=Bt, scale=0.7, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert A.info().transpose_built == 0 and not bool(torch.isnan(dQ).any()) and not bool(torch.isnan(dB).any())
    assert A.buildTranspose() == 0, _capi.last_error()
    full = _edge(A, mat, Q, K, V, dO, Bt, scale=0.7)
    assert _same(dQ, full[1]) and _same(dB, full[4])  # alone they have the bits they have with the rest
    # k = 0: every score is the bias alone -- the bits of Q = +0 at k = 4 (qk = +0 either way)
    Q0, K0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.m, mat.n))
    O0, dV0, dB0 = _nan(O.shape, O), _nan(V.shape, V), _nan(Bt.shape, Bt)
    assert A.mhaEdgeBias(Q0, K0, V, O0, B=Bt, scale=0.7) == 0, _capi.last_error()
    assert A.mhaEdgeBiasBackward(Q0, K0, V, dO, dV=dV0, work=_work(mat, Q), B=Bt, scale=0.7, dB=dB0) == 0, _capi.last_error()
    torch.cuda.synchronize()
    zeroed = _edge(A, mat, torch.zeros_like(Q), K, V, dO, Bt, scale=0.7)
    assert _same(O0, zeroed[0]) and _same(dV0, zeroed[3]) and _same(dB0, zeroed[4])
    # d = 0 in the backward: dB is the score gradient of an empty product, +0 wherever p is finite
    V0, dO0 = (torch.zeros((r, 3, 0), dtype=_tdt(dtype), device=DEV) for r in (mat.n, mat.m))
    dB = _nan(Bt.shape, Bt)
    assert A.mhaEdgeBiasBackward(Q, K, V0, dO0, B=Bt, dB=dB) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not _bits(dB.cpu().numpy()).any()
    _close(A)
    none = zoo.empty_matrix()  # nnz = 0: +0 everywhere, no element of dB
    A = _open(none, np.zeros(0), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(none, 3, 4, 6, dtype, seed=1812)
    for t in _edge(A, none, Q, K, V, dO, torch.zeros((0, 3), dtype=_tdt(dtype), device=DEV), scale=2.0):
        assert not _bits(t.cpu().numpy()).any()
    _close(A)


# ---- 9. graph replay ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_both_calls_replay_from_a_graph(dtype):
    """one forward and one backward, captured on a single linear stream that has run them once before; replayed after B changed
    in place"""
    mat = _zoo()["half-empty"]
    A = _open(mat, np.ones(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Bt = _dev(EB.distinct_bias(mat, 3, 1820), dtype)
    Q, K, V, dO = _operands(mat, 3, 5, 6, dtype, seed=1821)
    O = torch.full((mat.m, 3, 6), POISON, dtype=_tdt(dtype), device=DEV)
    outs = [torch.full(t.shape, POISON, dtype=t.dtype, device=DEV) for t in (Q, K, V)]
    dB = torch.full((mat.nnz, 3), POISON, dtype=_tdt(dtype), device=DEV)
    work = torch.empty(12 * mat.m, dtype=Q.dtype, device=DEV)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert A.setStream(side) == 0

    def both():
        assert A.mhaEdgeBias(Q, K, V, O, B=Bt, scale=0.4) == 0, _capi.last_error()
        assert A.mhaEdgeBiasBackward(Q, K, V, dO, outs[0], outs[1], outs[2], work, B=Bt, scale=0.4, dB=dB) == 0, _capi.last_error()
    with torch.cuda.stream(side):
        both()  # (the stream has run the calls once before the capture)
    torch.cuda.synchronize()
    held = A.info().device_bytes
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both()
    assert A.info().device_bytes == held
    torch.cuda.synchronize()
    Bn = _dev(EB.distinct_bias(mat, 3, 1822), dtype)
    assert not _same(Bn, Bt)
    Bt.copy_(Bn)  # changed in place: the graph reads the same address
    for t in [O] + outs + [dB]:
        t.fill_(POISON)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in [O] + outs + [dB]]
    del graph
    assert A.setStream(None) == 0
    for g, e in zip(replayed, _edge(A, mat, Q, K, V, dO, Bn, scale=0.4)):
        assert _same(g, e)
    _close(A)


# ---- 10. autograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_autograd_gradients_match_the_float64_reference_and_the_handle_keeps_its_values(dtype):
    for which in ("random", "class-edges"):
        mat = _zoo()["class-edges"] if which == "class-edges" else EB.random_matrix()
        rows, cols = _index(mat)
        Bt, c, (Q, K, V, dO) = _case_f(mat, dtype, EB.F_SEEDS[which] + 5)
        A = _open(mat, np.random.default_rng(1900).uniform(-1, 1, size=mat.nnz), dtype)
        stored, key = A._arrays[2].clone(), getattr(A, "_autograd_key", None)
        q, k_, v, b = (t.clone().requires_grad_(True) for t in (Q, K, V, Bt))
        out = autograd.multihead_attention(A, q, k_, v, scale=1 / np.sqrt(EB.F_K), bias=b)
        out.backward(dO)
        torch.cuda.synchronize()
        assert getattr(A, "_autograd_key", None) is key and _same(A._arrays[2], stored)  # the handle's values are what they were
        direct = _edge(A, mat, Q, K, V, dO, Bt, scale=1 / np.sqrt(EB.F_K))
        assert _same(A._arrays[2], stored)
        assert b.grad.shape == Bt.shape and _same(b.grad, direct[4])  # grad_bias IS dB
        for g, w in zip((out.detach(), q.grad, k_.grad, v.grad), direct[:4]):
            assert _same(g, w)
        want = EB.reference(mat, rows, cols, c, Bt, Q, K, V, dO)
        allow = EB.allowances(mat, rows, cols, c, Bt, Q, K, V, dO, dtype, STAGES)
        assert STAGES * allow[0] <= FIRST_ORDER
        for g, w, al, what in zip((out.detach(), q.grad, k_.grad, v.grad, b.grad), want, allow[1:], NAMES):
            _within(g, w, al, f"{mat.name} {_dt(dtype)} autograd {what}")
        # no gradient for the bias: no dB is formed; a bias that is a strided slice is taken as it is
        wide = torch.zeros((mat.nnz, EB.F_HEADS + 2), dtype=Bt.dtype, device=DEV)
        wide[:, :EB.F_HEADS] = Bt
        q2 = Q.clone().requires_grad_(True)
        out2 = autograd.multihead_attention(A, q2, K, V, scale=1 / np.sqrt(EB.F_K), bias=wide[:, :EB.F_HEADS])
        out2.backward(dO)
        torch.cuda.synchronize()
        assert _same(out2.detach(), direct[0]) and _same(q2.grad, direct[1])
        with pytest.raises(ValueError, match="slopes"):
            autograd.multihead_attention(A, Q, K, V, bias=Bt, slopes=torch.ones(EB.F_HEADS, dtype=Bt.dtype, device=DEV))
        # a 1-D bias is the old route: it still leaves the handle holding the bias
        one = Bt[:, 0].contiguous()
        autograd.multihead_attention(A, Q, K, V, bias=one)
        torch.cuda.synchronize()
        assert A._autograd_key is not None and A._autograd_val.data_ptr() == one.data_ptr()
        assert not _same(A._arrays[2], stored)
        _close(A)
