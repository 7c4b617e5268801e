"""``mhaBiased`` / ``mhaBiasedBackward`` on the GPU where tests/test_gpu_mha_bias.py does not reach: the 16-byte-load
instantiations with a real bias AND a real scale, every conversion path, head groups of three and of all heads, rows alone,
non-finite values under slopes, and the float64 reference at the class edges (the patterns of tests/attention_edges.py).

A  16-byte loads, exact by augmentation.  k = 12 widened to 12 + 1 + 3 = 16: ``mha`` / ``mhaBackward`` on c Q | u | 0 and
   K | slope v | 0 (tests/mha_bias_reference.py: ``augment`` for the padding and the sign of zero, ``scaled_identity`` for the
   power-of-two scale).  WHY THESE WIDTHS.  The summation order of dQ and dK is a function of (L, width): 12 and 16 round up to the
   same power of two, 16, so the first 12 columns of a gradient of width 16 are summed as a gradient of width 12 is.  The load
   width: 12 and 16 values are a multiple of 16 bytes in both types (48 | 96 and 64 | 128), as are d = 8 values, and k is at
   least one block of 32 bytes; the operands are contiguous allocations.  So ``attention_vec`` and ``attention_bwd_vec`` hold on
   BOTH sides, in both types, which the test asserts from the transcribed rule (tests/test_mha_bias_host.py checks the
   transcription against the headers' functions): where tests/test_gpu_mha_bias.py (C) forces element loads, this one cannot
   fall back to them unnoticed.
B  the same bits on every path and sigma, with a distinct value in every entry: the biased kernels are the one consumer of the
   tile-ordered VALUE array through the rank -> storage rule.
C  head h of every output, and column h of dS, is the single-head biased call on the slices -- with groups of three heads and of
   all heads, which no other biased test runs.
D  a row alone in a one-row matrix at another sigma has the bits it has inside the matrix.
E  b = slopes[h] * a is one IEEE multiplication: 0 * -Inf is NaN, -1 * -Inf is +Inf, a NaN value poisons its row in every head.
F  the float64 reference and the allowance of tests/test_gpu_mha_bias.py, unchanged, on class-edges and its transpose.

No tolerance is introduced here: A to E compare bits, F uses the derived allowance of that file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import attention_edges as E  # noqa: E402
from tests import mha_bias_reference as B  # noqa: E402
from tests import sddmm_reference as S  # noqa: E402
from tests.test_gpu_attention_autograd import FIRST_ORDER, STAGES, _index, _within  # noqa: E402
from tests.test_gpu_attention_backward import SIGMA_PATHS  # noqa: E402
from tests.test_gpu_attention_edges import GROUP_CASES, _mat, _padded  # noqa: E402
from tests.test_gpu_exact_reference import DEV, PATHS, _close, _handle  # noqa: E402
from tests.test_gpu_mha_bias import (AUTO, _bias_allowances, _biased, _dev, _dt, _mask, _nan, _open, _operands, _plain,  # noqa: E402
                                     _reference, _same, _tdt, _written, _zoo)

NAMES = ("O", "dQ", "dK", "dV", "dS")
ALONE = (15, 61, 256, 511, 768)


def _sl(slopes, dtype):
    return None if slopes is None else _dev(np.array(slopes), dtype)


def _size(dtype):
    return np.dtype(dtype).itemsize


def _vec_both(heads, k, d, dtype, Q, K, V, dO):
    """the host-side rule on these very tensors: (forward, backward) take 16-byte loads"""
    ld = lambda t: int(t.stride(0))  # noqa: E731
    return (B.vec_forward(heads, k, _size(dtype), ld(Q), ld(K), Q.data_ptr(), K.data_ptr()),
            B.vec_backward(heads, k, d, _size(dtype), [ld(t) for t in (Q, K, V, dO)], [t.data_ptr() for t in (Q, K, V, dO)]))


# ---- A. 16-byte loads with a real bias and a real scale -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("sigma", (AUTO, 4), ids=("auto", "sigma4"))
@pytest.mark.parametrize("name", ("two-hubs", "class-edges", "dealt"))
def test_sixteen_byte_loads_with_a_rank_one_bias_and_a_scale_have_the_bits_of_mha_on_widened_operands(name, sigma, dtype):
    """The identity (module docstring, tests/mha_bias_reference.py): with a_e = u_i v_j and c a power of two,
        O, dV = those of mha / mhaBackward on c Q | u | 0, K | slope v | 0,
        dK    = the first 12 columns of the widened dK (sum (ds c) Q = sum ds (c Q)),
        dQ    = c times the first 12 columns of the widened dQ (sum (ds c) K = c sum ds K),
    bit for bit while no c x is subnormal.  That is asserted on the data: c Q is far from the subnormals; every softmax weight is
    at least exp(-(spread + ln L)) >= 2**10 smallest normals (``score_spread``), so p and the chains it enters are normal; and
    every non-zero ds c of the call's own dS (whose bits tests/test_gpu_mha_bias.py (D) pins) is a normal number, so t = ds c
    is exact.  A column kernel computing (qk + b) c, dropping the slope or keeping the first head's slope changes bits of the
    scores (tests/test_mha_bias_host.py evaluates those wrong scores on these operands) and with them dK and dV here."""
    mat = _zoo()[name]
    heads, k, d, kw = B.A_HEADS, B.A_K, B.A_D, B.A_K + 1 + B.A_PAD
    assert (heads, k, kw, d) == (3, 12, 16, 8) and E.heads_per_group(mat.m, heads) == 2
    u, v, a = B.rank_one(mat, seed=7)
    A = _open(mat, a, dtype, sigma)
    assert A.buildTranspose() == 0, _capi.last_error()
    Qn, Kn, Vn, dOn = B.operands_a(mat, dtype)
    Q, K, V, dO = (_dev(t, dtype) for t in (Qn, Kn, Vn, dOn))
    assert all(t.is_contiguous() for t in (Q, K, V, dO)) and _vec_both(heads, k, d, dtype, Q, K, V, dO) == (True, True)
    rows, cols = B.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    qk = (Qn[rows].astype(np.float64) * Kn[cols]).sum(axis=2)
    floor = -np.log(float(np.finfo(dtype).tiny)) - 7
    for scale in B.A_SCALES:
        c = B.scaled_identity(scale)
        for slopes in (None, B.A_SLOPES):
            what = (name, A.info().sigma, scale, slopes)
            got = _biased(A, mat, Q, K, V, dO, scale=scale, slopes=_sl(slopes, dtype))
            _written(got, what)
            b = (np.ones(heads) if slopes is None else np.array(slopes))[None, :] * a[:, None]
            if c != 1:  # (a multiplication by 1 is exact whatever its operand)
                assert B.no_subnormal(Qn, c) and B.score_spread(mat, c, qk, b) <= floor, what
                assert B.no_subnormal(got[4].cpu().numpy(), c, margin=1), what
            Qw, Kw = (_dev(t, dtype) for t in B.augment(Qn * dtype(c), Kn, u, v, slopes, pad=B.A_PAD))
            assert Qw.shape[2] == kw and _vec_both(heads, kw, d, dtype, Qw, Kw, V, dO) == (True, True)
            O, dQw, dKw, dV = _plain(A, mat, Qw, Kw, V, dO)
            for g, w, n in zip(got, (O, dQw[:, :, :k] * c, dKw[:, :, :k], dV), NAMES):
                assert _same(g, w), what + (n,)
    _close(A)


# ---- B. every path and sigma -------------------------------------------------------------------------------------------------------
def _path_operands(mat, dtype):
    return _operands(mat, 3, 8, 16, dtype, seed=1201), _dev(np.array([0.7, -1.3, 0.11]), dtype)


def _both_calls(A, mat, ops, slopes, what):
    got = _biased(A, mat, *ops, scale=0.37, slopes=slopes)
    _written(got, what)
    return [g.cpu().numpy() for g in got]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_same_bits_on_every_path_and_sigma_with_a_distinct_value_in_every_entry(dtype):
    """No bit of the five outputs depends on the conversion: every path of tests/test_gpu_exact_reference.py and sigma 4, 7, 16
    and 32, each with its companion, gives the bits of the first.  The values are a permutation of nnz equidistant numbers, so a
    value read at another entry's position is an error of order one.  Asserted among the configurations: a fast-track tile and
    tiles in tile order (the oracle's conversion at the handle's sigma, p compared with the handle's), a non-empty tail, a slab
    path, a hot table, and two different companions."""
    from oracle.csr5_oracle import Oracle
    mat = _zoo()["class-edges"]
    val = B.distinct_values(mat, 1200)
    ops, slopes = _path_operands(mat, dtype)
    orc, structure = Oracle(), {}
    first, seen, companions = None, dict(fast=False, moved=False, tail=False, slabs=False, hot=False), set()
    for path in PATHS + SIGMA_PATHS:
        A, _ = _handle(mat, val, path, dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        info = A.info()
        got = _both_calls(A, mat, ops, slopes, path.name)
        _close(A)
        first = first or got
        for g, w, n in zip(got, first, NAMES):
            assert E.same_bits(g, w), (path.name, n)
        if info.sigma not in structure:
            fmt = orc.convert(64, info.sigma, mat.m, mat.row_ptr, mat.col, val)
            structure[info.sigma] = (fmt.p,) + B.tile_structure(fmt, mat.nnz)
        p, fast, tail = structure[info.sigma]
        assert p == info.p and info.transpose_built == 1, path.name
        seen["fast"] |= fast > 0
        seen["moved"] |= fast < p - 1
        seen["tail"] |= tail > 0
        seen["slabs"] |= info.column_slabs > 0
        seen["hot"] |= info.slab_hot == 1
        companions.add((info.t_sigma, info.t_column_slabs))
        print(f"{path.name}: sigma {info.sigma} p {info.p} fast-track {fast} tail {tail} slabs {info.column_slabs} hot {info.slab_hot} "
              f"companion sigma {info.t_sigma} slabs {info.t_column_slabs} hot {info.t_slab_hot}")
    assert all(seen.values()), seen
    assert len(companions) >= 2, companions


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_new_values_reach_both_sides_on_a_slab_path_and_on_a_plain_one(dtype):
    """buildTranspose, then updateValues with a second permutation: all five outputs have the bits of a fresh handle on the new
    values -- on slabs8-hot, where spmv reads the slab children's values and not the tile-ordered array the biased kernels read,
    and on the default path"""
    mat = _zoo()["class-edges"]
    old, new = B.distinct_values(mat, 1200), B.distinct_values(mat, 1201)
    ops, slopes = _path_operands(mat, dtype)
    by_name = {p.name: p for p in PATHS}
    A, _ = _handle(mat, new, by_name["fused-default"], dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    fresh = _both_calls(A, mat, ops, slopes, "fresh")
    _close(A)
    slabbed = 0
    for name in ("slabs8-hot", "fused-default"):
        A, _ = _handle(mat, old, by_name[name], dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        before = _both_calls(A, mat, ops, slopes, name)
        assert not E.same_bits(before[0], fresh[0])
        assert A.updateValues(_dev(new, dtype)) == 0, _capi.last_error()
        info = A.info()
        slabbed += info.column_slabs > 0 and info.slab_hot == 1 and info.t_column_slabs > 0  # (the companion runs on slabs too)
        print(f"{name}: slabs {info.column_slabs} hot {info.slab_hot} companion slabs {info.t_column_slabs} hot {info.t_slab_hot}")
        for g, w, n in zip(_both_calls(A, mat, ops, slopes, name), fresh, NAMES):
            assert E.same_bits(g, w), (name, n)
        _close(A)
    assert slabbed == 1


# ---- C. every head is the single-head biased call ------------------------------------------------------------------------------
def _per_head_biased(A, mat, Q, K, V, dO, scale, slopes):
    """[O, dQ, dK, dV, dS] from heads = 1 calls on the slices [:, h:h + 1], slopes[h:h + 1] and a dS of leading dimension 1"""
    heads = Q.shape[1]
    O = _nan((mat.m,) + tuple(V.shape[1:]), V)
    outs = [_nan(t.shape, t) for t in (Q, K, V)]
    dS = _nan((mat.nnz, heads), Q)
    work = torch.empty(4 * mat.m, dtype=Q.dtype, device=DEV)
    for h in range(heads):
        s = slice(h, h + 1)
        sl = None if slopes is None else slopes[s]
        ds = _nan((mat.nnz, 1), Q)
        assert A.mhaBiased(Q[:, s], K[:, s], V[:, s], O[:, s], scale=scale, slopes=sl) == 0, _capi.last_error()
        assert A.mhaBiasedBackward(Q[:, s], K[:, s], V[:, s], dO[:, s], outs[0][:, s], outs[1][:, s], outs[2][:, s], work, scale=scale,
                                   slopes=sl, dS=ds) == 0, _capi.last_error()
        dS[:, h] = ds[:, 0]
    torch.cuda.synchronize()
    return [O] + outs + [dS]


def _slopes_for(heads, dtype):
    return _dev(np.random.default_rng([1400, heads]).uniform(-1.5, 1.5, size=heads), dtype)


assert {c[2] for c in GROUP_CASES} >= {3} and any(c[2] == c[1] and c[1] >= 3 for c in GROUP_CASES)


@pytest.mark.parametrize("side", ("", "^T"), ids=("rows", "transposed"))
@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: f"m{c[0]}-h{c[1]}-k{c[3]}-d{c[4]}-{_dt(c[5])}")
def test_every_head_of_a_wide_group_is_the_single_head_biased_call(case, side):
    """Groups of 3 + 3 + 2 heads and of all heads: a lane of a short line keeps its value across the heads of the group, longer
    lines read it again per head, the slopes and dS advance by the head in the backward.  Head h must not see any of that: the
    call with heads = 1 on the slices computes the same chains (the definition is per head), so the bits agree.  k and d are
    the cases' own: at (k, d) = (3, 5) both calls take element loads; at (8, 4) both take 16-byte loads (every slice starts on
    a multiple of 32 bytes) -- and where they differed the contract would still ask for equality: either load width feeds the
    same chains."""
    m, heads, hper, k, d, dtype = case
    mat = _mat(f"many-lines-{m}{side}")
    assert mat.m == mat.n == m and E.heads_per_group(m, heads) == hper and hper in (3, heads) and hper >= 3
    val = B.distinct_values(mat, 1401)
    A = _open(mat, val, dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, heads, k, d, dtype, seed=1402)
    slopes = _slopes_for(heads, dtype)
    got = _biased(A, mat, Q, K, V, dO, scale=0.37, slopes=slopes)
    _written(got, (m, side, heads))
    for g, w, n in zip(got, _per_head_biased(A, mat, Q, K, V, dO, 0.37, slopes), NAMES):
        assert _same(g, w), (m, side, heads, n)
    _close(A)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_every_head_at_the_class_edges_is_the_single_head_biased_call(dtype):
    """class-edges and its transpose, heads = 3 (groups of two and one): (8, 16) with 16-byte loads in both calls, and a width
    whose slices are NOT all aligned (k = 10 in fp32, 5 in fp64, in rows of 32 resp. 16 values): the packed call takes element
    loads, the single-head call 16-byte loads for heads 0 and 2 and element loads for head 1 -- the same chains, the same
    bits.  heads = 1 without slopes on a handle of zeros is ``mha`` / ``mhaBackward`` with one head."""
    size = _size(dtype)
    for name in ("class-edges", "class-edges^T"):
        mat = _mat(name)
        A = _open(mat, B.distinct_values(mat, 1410), dtype)
        assert A.buildTranspose() == 0, _capi.last_error()
        slopes = _slopes_for(3, dtype)
        for k, d, extra in ((8, 16, 0), (40 // size, 6, 8 // size)):
            Q, K, V, dO = _operands(mat, 3, k, d, dtype, seed=1411)
            Q, K = _padded(Q, extra), _padded(K, extra)
            packed = _vec_both(3, k, d, dtype, Q, K, V, dO)
            single = [B.vec_forward(1, k, size, int(Q.stride(0)), int(K.stride(0)), Q[:, h:].data_ptr(), K[:, h:].data_ptr()) for h in range(3)]
            assert (packed, single) == (((True, True), [True] * 3) if extra == 0 else ((False, False), [True, False, True]))
            got = _biased(A, mat, Q, K, V, dO, scale=0.37, slopes=slopes)
            _written(got, (name, k, d))
            for g, w, n in zip(got, _per_head_biased(A, mat, Q, K, V, dO, 0.37, slopes), NAMES):
                assert _same(g, w), (name, k, d, n)
        _close(A)
    mat = _mat("class-edges")
    A = _open(mat, np.zeros(mat.nnz), dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    Q, K, V, dO = _operands(mat, 1, 8, 16, dtype, seed=1412)
    got = _biased(A, mat, Q, K, V, dO)
    _written(got, "heads = 1")
    for g, w, n in zip(got, _plain(A, mat, Q, K, V, dO), NAMES):
        assert _same(g, w), ("heads = 1", n)
    _close(A)


# ---- D. a biased row alone -------------------------------------------------------------------------------------------------------
def _row_calls(A, mat, Q, K, V, dO, slopes):
    """[O, dQ, dS] without companion and workspace"""
    O, dQ, dS = _nan((mat.m,) + tuple(V.shape[1:]), V), _nan(Q.shape, Q), _nan((mat.nnz, Q.shape[1]), Q)
    assert A.mhaBiased(Q, K, V, O, scale=0.37, slopes=slopes) == 0, _capi.last_error()
    assert A.mhaBiasedBackward(Q, K, V, dO, dQ=dQ, scale=0.37, slopes=slopes, dS=dS) == 0, _capi.last_error()
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(t).any()) for t in (O, dQ, dS)), "an element was not written"
    return [t.cpu().numpy() for t in (O, dQ, dS)]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_biased_edge_row_alone_gives_the_bits_it_has_inside_the_matrix(dtype):
    """rows 15 (63 entries, a wavefront's), 61 (2 049, beside a hub of 2 048), 256 (4 097, first of workgroup 1), 511 (513, last of
    workgroup 1) and 768 (600, alone in workgroup 3), each as the one row of a matrix at sigma = 7 with its own slice of the
    values: a row's O, dQ and dS are functions of the row alone (its entries in CSR order, its values, its operands), not of the
    workgroup, the tile or the storage position it is read from"""
    mat = _mat("class-edges")
    lens = np.diff(mat.row_ptr)
    assert [int(lens[r]) for r in ALONE] == [63, 2049, 4097, 513, 600]
    val = B.distinct_values(mat, 1500)
    Q, K, V, dO = _operands(mat, 3, 8, 16, dtype, seed=1501)
    slopes = _slopes_for(3, dtype)
    A = _open(mat, val, dtype)
    O, dQ, dS = _row_calls(A, mat, Q, K, V, dO, slopes)
    _close(A)
    for r in ALONE:
        a, b = int(mat.row_ptr[r]), int(mat.row_ptr[r + 1])
        one = M.CsrMatrix(1, mat.n, np.array([0, b - a], dtype=np.int32), mat.col[a:b].copy(), val[a:b].copy(), f"row{r}")
        A1 = _open(one, val[a:b], dtype, 7)
        O1, dQ1, dS1 = _row_calls(A1, one, Q[r:r + 1].clone(), K, V, dO[r:r + 1].clone(), slopes)
        _close(A1)
        assert E.same_bits(O1[0], O[r]), (r, "O")
        assert E.same_bits(dQ1[0], dQ[r]), (r, "dQ")
        assert E.same_bits(dS1, dS[a:b]), (r, "dS")


# ---- E. non-finite values under slopes ---------------------------------------------------------------------------------------------
E_SLOPES = (1.0, 0.0, -1.0)


def _e_operands(mat, dtype, seed):
    """Q = 0 (qk = +0: the score is the bias), K uniform, V and dO integers (so the finite expectations are exact in any order)"""
    heads, k, d = 3, 3, 5
    rng = np.random.default_rng(seed)
    Kn = rng.uniform(-1, 1, size=(mat.n, heads, k)).astype(dtype)
    Vn = rng.integers(-1000, 1001, size=(mat.n, heads, d)).astype(dtype)
    dOn = rng.integers(-8, 9, size=(mat.m, heads, d)).astype(dtype)
    Q = torch.zeros((mat.m, heads, k), dtype=_tdt(dtype), device=DEV)
    return Q, _dev(Kn, dtype), _dev(Vn, dtype), _dev(dOn, dtype), Vn, dOn


def _run_e(mat, values, dtype, ops):
    A = _open(mat, values, dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    got = _biased(A, mat, *ops, scale=0.5, slopes=_dev(np.array(E_SLOPES), dtype))
    _close(A)
    return [g.cpu().numpy() for g in got]


def _nan_lines(t):
    """(lines that are NaN in every element, lines that hold a NaN) of a (lines, width) array"""
    n = np.isnan(t)
    return n.all(axis=1), n.any(axis=1)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
def test_a_mask_under_slopes_one_zero_and_minus_one(dtype):
    """values 0 or -Inf, slopes (1, 0, -1), Q = 0.  Head 0 is the hard mask of tests/test_gpu_mha_bias.py (E).  Head 1: 0 * -Inf
    is NaN, so exactly the rows that hold a masked entry are NaN; head 2: -1 * -Inf = +Inf, a +Inf score makes M = +Inf and
    s - M NaN, so exactly those rows are NaN too.  In both, a row without masked entry has b = 0 * 0 = +0 resp. -1 * 0 = -0,
    s = fma(+0, c, b) = +0 in every entry: the mean of its V rows, exactly; dV sums dO / L over those rows' entries (dyadic for
    the lengths 1 and 16 such rows have), and the columns a NaN row stores are NaN in dK and dV."""
    mat = _zoo()["class-edges"]
    keep = _mask(mat, 600)
    mixed, dead = E.mask_conditions(mat, keep)
    assert mixed and 0 < dead < 0.5
    Q, K, V, dO, Vn, dOn = _e_operands(mat, dtype, 1600)
    O, dQ, dK, dV, dS = _run_e(mat, np.where(keep, 0.0, -np.inf), dtype, (Q, K, V, dO))
    rows, cols = E.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    lens = np.diff(mat.row_ptr)
    kept = np.bincount(rows[keep], minlength=mat.m)
    dead_rows = (lens > 0) & (kept == 0)
    masked_rows = kept < lens
    whole = (lens > 0) & ~masked_rows
    assert set(lens[whole].tolist()) == {1, 16} and dead_rows.any() and (masked_rows & ~dead_rows).any()
    for h in range(3):
        nan_rows = dead_rows if h == 0 else masked_rows
        unmasked = keep if h == 0 else ~masked_rows[rows]
        want, mag = E.exact_forward(mat, Vn[:, h], unmasked, dtype)
        assert mag < E.EXACT_LIMIT
        if h:
            want[masked_rows] = np.nan
        assert E.same_bits(O[:, h], want), (h, "O")
        for t, n in ((O[:, h], "O"), (dQ[:, h], "dQ")):
            every, some = _nan_lines(t)
            assert np.array_equal(every, nan_rows) and np.array_equal(some, nan_rows), (h, n)
        every, some = _nan_lines(dS[:, h:h + 1])
        assert np.array_equal(some, nan_rows[rows]), (h, "dS")
        live = unmasked & ~nan_rows[rows]
        count = (kept if h == 0 else lens)[rows[live]]
        want = np.zeros((mat.n, dOn.shape[2]))
        np.add.at(want, cols[live], dOn[rows[live], h].astype(np.float64) / count[:, None])
        poisoned = np.zeros(mat.n, dtype=bool)
        poisoned[cols[nan_rows[rows]]] = True
        want[poisoned] = np.nan
        assert E.same_bits(dV[:, h], want.astype(dtype)), (h, "dV")
        every, some = _nan_lines(dK[:, h])
        assert np.array_equal(every, poisoned) and np.array_equal(some, poisoned), (h, "dK")


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "plus-inf"))
def test_one_non_finite_value_stays_in_its_row_and_its_columns(bad, dtype):
    """one entry of a row of each class (15, 511, 2 048 and 4 097 entries) gets the value, every other value is +0, slopes
    (1, 0, -1), Q = 0.  NaN: slope * NaN is NaN in every head, so exactly those four rows are NaN in all heads of O and dQ, exactly
    the columns they store in dK and dV, exactly their entries in dS.  +Inf: the same in heads 0 and 1 (a +Inf score; 0 * Inf is
    NaN), while in head 2 the bias is -1 * +Inf = -Inf, a MASK: the row stays finite, O is exactly the mean of the other entries'
    V rows and the entry's own dS is zero.  Everything else has the bits of the run with all values +0."""
    mat = _zoo()["class-edges"]
    lens = np.diff(mat.row_ptr)
    hit_rows = [int(np.flatnonzero(lens == L)[0]) for L in (15, 511, 2048, 4097)]
    entries = np.array([int(mat.row_ptr[r]) + int(lens[r]) // 3 for r in hit_rows])
    rows, cols = E.rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    Q, K, V, dO, Vn, _ = _e_operands(mat, dtype, 1610)
    base = _run_e(mat, np.zeros(mat.nnz), dtype, (Q, K, V, dO))
    assert not any(np.isnan(t).any() for t in base)
    values = np.zeros(mat.nnz)
    values[entries] = bad
    got = _run_e(mat, values, dtype, (Q, K, V, dO))
    hit = np.zeros(mat.m, dtype=bool)
    hit[hit_rows] = True
    stored = np.zeros(mat.n, dtype=bool)
    stored[cols[hit[rows]]] = True
    assert 0 < stored.sum() < mat.n
    lines = (hit, hit, stored, stored, hit[rows])
    for h in range(3):
        masks = bad > 0 and h == 2  # (+Inf under the slope -1: a mask, no NaN)
        for g, w, where, n in zip(got, base, lines, NAMES):
            gh, wh = (g[:, h:h + 1], w[:, h:h + 1]) if n == "dS" else (g[:, h], w[:, h])
            assert E.same_bits(gh[~where], wh[~where]), (h, n, "beside the rows")
            every, some = _nan_lines(gh[where])
            assert not some.any() if masks else every.all(), (h, n)
        if masks:
            unmasked = np.ones(mat.nnz, dtype=bool)
            unmasked[entries] = False
            want, mag = E.exact_forward(mat, Vn[:, h], unmasked, dtype)
            assert mag < E.EXACT_LIMIT
            assert E.same_bits(got[0][:, h], want), "O with the entries masked"
            assert not got[4][entries, h].any() and got[4][hit[rows], h].any()


# ---- F. the float64 reference at the class edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", S.DTYPES, ids=_dt)
@pytest.mark.parametrize("ki", (0, 1), ids=lambda i: f"k{B.F_KD[i][0]}-d{B.F_KD[i][1]}")
@pytest.mark.parametrize("mi", (0, 1), ids=("class-edges", "class-edges^T"))
def test_biased_calls_match_the_float64_reference_at_the_class_edges(mi, ki, dtype):
    """rows (and, transposed, columns) of 2 049, 4 096 and 4 097 entries against torch autograd in float64, with the allowance of
    tests/test_gpu_mha_bias.py as it is.  Its condition STAGES rho <= FIRST_ORDER holds with values in [-2, 2) and Q in [-2, 2):
    rho is at most 4.94e-4 (fp32, class-edges, k = 8; 1.84e-12 in fp64), 1.04e-5 on the transpose (3.81e-14), evaluated in numpy
    by tests/test_mha_bias_host.py -- nothing was shrunk."""
    mat = _mat(("class-edges", "class-edges^T")[mi])
    k, d = B.F_KD[ki]
    rows, cols = _index(mat)
    valn, slopesn, c, ops = B.case_f(mat, k, d, dtype, 1300 + 10 * mi + 2 * ki)
    val, slopes = _dev(valn, dtype), _dev(slopesn, dtype)
    Q, K, V, dO = (_dev(t, dtype) for t in ops)
    A = _open(mat, valn, dtype)
    assert A.buildTranspose() == 0, _capi.last_error()
    got = _biased(A, mat, Q, K, V, dO, scale=1 / np.sqrt(k), slopes=slopes)
    _close(A)
    _written(got, mat.name)
    want = _reference(mat, rows, cols, c, val, slopes, Q, K, V, dO)
    allow = _bias_allowances(mat, rows, cols, c, val, slopes, Q, K, V, dO, dtype)
    what = f"{mat.name} {_dt(dtype)} k={k} d={d}"
    print(f"{what}: rho {allow[0]:.3e}")
    assert STAGES * allow[0] <= FIRST_ORDER, (what, allow[0])
    for g, w, a, n in zip(got, want, allow[1:], NAMES):
        _within(g, w, a, f"{what} {n}")
