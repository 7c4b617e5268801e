"""What the conversion builds for the hot slab child, array by array, against a host model of the rule (tests/slab_child_reference.py, pinned
down by tests/test_slab_child_reference_host.py).  y cannot see most of it: any monotone cut table, any table content, any cold order gives
the same y.  Here every array csr5hip_get_slab_view exposes -- slab offsets, first tiles, table columns, cold regions, packed codes, the plain
child CSR, the values through the piece layout, the tiles' prefix costs, the cut table, the range heads, the permuted copy of x -- must EQUAL
the model's (integers and bit patterns, no tolerance), and a failure names the array and the first index.  The same run checks y on integer
data against the oracle, so that a structure failure and a y failure can be told apart.

Every case: setColumnSlabs(S), setSlabHot(2), setSigma(16); stride == 1 (the use counts are exact: the model does not restate the sample).
Matrices: the five extremes of test_gpu_range_cuts.py (fp64, fp32); tables with more candidates than slots (fp64: 16 384 slots, fp32: 32 768),
where the threshold rises above min_count and the second class is contested; other (S, shift) maps; slabs without a column."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests import slab_child_reference as R  # noqa: E402
from tests.test_gpu_parity import DEV, Y_POISON, _device_csr  # noqa: E402
from tests.test_gpu_range_cuts import MATRICES, _from_lengths, hub_rows_then_short_rows  # noqa: E402
from tests.test_gpu_slabs import _hub_columns_matrix  # noqa: E402
from tests.test_range_cut_host import DEFAULT_SLOTS, rule_cuts  # noqa: E402

SIGMA = 16
HOT_LDS_BYTES = 128 * 1024  # csr5_slab_plan.h: the table's share of the LDS -> 16 384 fp64 / 32 768 fp32 slots
MIN_COUNT = 16              # csr5_slab_plan.h: 16 / stride uses earn a slot


@functools.lru_cache(maxsize=None)
def overfull_tables(per_slab):
    """8 slabs (shift 4) x per_slab columns -- local ids 0 .. per_slab-1 of every slab --, each used 16 to 19 times (15 / 30 / 35 / 20 %), in
    random order over rows of 24 non-zeros on average.  per_slab = 22 000 against 16 383 usable slots: 55 % of the columns are used 18 times
    or more and fit, 85 % are used 17 times or more and do not -> thr 18, and the 6 600 columns of 17 uses compete for some 4 300 slots."""
    rng = np.random.default_rng(per_slab)
    cols = np.concatenate([R.slab_column(k, np.arange(per_slab), 4, 3) for k in range(8)])
    uses = rng.choice([16, 17, 18, 19], p=[0.15, 0.30, 0.35, 0.20], size=cols.size)
    col = rng.permutation(np.repeat(cols, uses))
    m = col.size // 24
    return _from_lengths(rng.multinomial(col.size, np.full(m, 1.0 / m)), col, int(cols.max()) + 1, f"overfull_{per_slab}")


@functools.lru_cache(maxsize=None)
def empty_slabs():
    """2 000 rows of 3 non-zeros in 40 columns: at S = 8, shift 4 only slabs 0 .. 2 own a column"""
    rng = np.random.default_rng(31)
    return _from_lengths([3] * 2000, rng.integers(0, 40, size=6000), 40, "empty_slabs")


@functools.lru_cache(maxsize=None)
def _model(make, arg, S, shift, value_size):
    mat = make(arg) if arg is not None else make()
    return R.build_model(mat.m, mat.n, mat.row_ptr, mat.col, S, shift, value_size, HOT_LDS_BYTES // value_size, MIN_COUNT)


def _int_values(mat, dtype, seed=5):
    val, x = M.fill_values(mat.nnz, mat.n, dtype, seed=seed, mode="int")
    if dtype == np.float32:  # (row sums stay far below 2^24: exact in fp32 too)
        val, x = (val % 3).astype(np.float32), (x % 3).astype(np.float32)
    return val, x


def _handle(mat, val, xd, dtype, S, shift, narrow=0):
    rp, ci, va = _device_csr(mat, val, dtype)
    A = H.anonymouslibHandle(mat.m, mat.n, dtype=np.dtype(dtype).name)
    A.keep = (rp, ci, va, xd)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0 and A.setX(xd) == 0 and A.setSigma(SIGMA) == 0
    assert A.setColumnSlabs(S) == 0 and A.setSlabShift(shift) == 0 and A.setSlabHot(2) == 0 and A.setNarrowValues(narrow) == 0
    assert A.asCSR5() == 0, _capi.last_error()
    return A


def _spmv(A, xd, m, dtype):
    y = torch.full((m,), Y_POISON, dtype=torch.float64 if dtype == np.float64 else torch.float32, device=DEV)
    assert A.setX(xd) == 0 and A.spmv(1.0, y) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _first(name, a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (name, int(bad[0]), a[bad[0]], b[bad[0]], int(bad.size))


def _check(oracle, mat, mo, dtype, S, shift, narrow=0):
    """converts, multiplies once, holds everything against the model `mo`; returns (device arrays, info)"""
    val, x = _int_values(mat, dtype)
    xd = torch.from_numpy(x).to(DEV)
    A = _handle(mat, val, xd, dtype, S, shift, narrow)
    info = A.info()
    assert info.slab_hot == 1 and info.column_slabs == S, (info.slab_hot, info.column_slabs)
    y = _spmv(A, xd, mat.m, dtype)
    dev = A.slab_child_arrays()
    if dev["stride"] != 1:
        pytest.skip("stride > 1: the use counts are sampled, the model does not restate which chunks are")
    assert dev["capacity"] == HOT_LDS_BYTES // np.dtype(dtype).itemsize and dev["min_count"] == MIN_COUNT
    found = R.compare(mo, dev)
    assert found == [], f"{mat.name}: (array, first index, model, device) {found}"
    # values, bit for bit, through the piece layout
    want = _bits(val.astype(dtype)[mo["order"]])
    _first("val", _bits(dev["val"])[mo["val_pos"][16 // np.dtype(dtype).itemsize]], want)
    assert dev["values_narrowed"] == (1 if narrow and dtype == np.float64 else 0) == info.slab_values_narrowed
    if dev["values_narrowed"]:
        _first("val32", _bits(dev["val32"])[mo["val_pos"][4]], _bits(val.astype(np.float32)[mo["order"]]))
    # the permuted copy of x after one spmv: table images over the slots in use, then the cold region
    cap = dev["capacity"]
    in_use = np.arange(cap)[None, :] < mo["hot_count"][:, None]
    _first("xperm (table images)", _bits(dev["xperm"][:S * cap].reshape(S, cap)[in_use]), _bits(x[mo["hot_cols"][in_use]]))
    _first("xperm (cold region)", _bits(dev["xperm"][S * cap:]), _bits(x[mo["cold_cols"]]))
    assert info.slab_hot_cover_pct == mo["cover_pct"] == R.slab_cover_pct(mo["covered"], 1, mat.nnz)
    assert info.slab_cold_entries == mo["cold_total"]
    # y, as the neighbouring tests check it: exact on integer data, rows without non-zeros in front of the CSR tail untouched
    exp = oracle.csr_spmv(mat.m, mat.row_ptr, mat.col, val, x)
    has = np.diff(mat.row_ptr) > 0
    _first("y", y[has], exp[has])
    assert np.all(y[:info.tail_partition_start][~has[:info.tail_partition_start]] == Y_POISON)
    assert A.destroy() == 0
    A.close()
    return dev, info


def _assert_foreign_elements(mo, dev):
    """an element whose column has a slot in its own slab but lies behind its tile's slab end is coded cold -- met, and the device agrees"""
    at = np.flatnonzero(mo["foreign_hot"])
    assert at.size > 0
    assert not np.any(dev["col_hi"][at] & 0x80) and not np.any(mo["col_hi"][at] & 0x80)
    assert np.any(np.asarray(mo["slab_off"][1:-1]) % mo["T"] != 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("make", MATRICES, ids=[f.__name__ for f in MATRICES])
def test_extremes_of_the_cuts(oracle, make, dtype):
    mat = make()
    mo = _model(make, None, 8, 4, np.dtype(dtype).itemsize)
    dev, _ = _check(oracle, mat, mo, dtype, 8, 4)
    if make is hub_rows_then_short_rows:  # the case tests the COST only if cutting by tile count would give another table
        by_count = np.array([mo["tile0"][k] + np.array(rule_cuts([1] * int(mo["tile0"][k + 1] - mo["tile0"][k]), DEFAULT_SLOTS, by_count=True))
                             for k in range(8)])
        assert np.any(by_count != dev["range_begin"])
        assert np.any(mo["tile_cold"] > 0) and np.any(mo["tile_cold"] == 0)


@pytest.mark.parametrize("per_slab,dtype", [(22000, np.float64), (44000, np.float32)], ids=["fp64_22000", "fp32_44000"])
def test_overfull_tables(oracle, per_slab, dtype):
    """more candidates than slots in every slab: threshold above min_count, a second class partly admitted in hash order, k_hot_rank over several
    groups of 1 024 x 128 columns... and in fp32 slots from 16 384 on (bit 14 of a code)"""
    mat = overfull_tables(per_slab)
    mo = _model(overfull_tables, per_slab, 8, 4, np.dtype(dtype).itemsize)
    cap = HOT_LDS_BYTES // np.dtype(dtype).itemsize
    for k, sel in enumerate(mo["selection"]):
        assert sel["thr"] > MIN_COUNT, (k, sel["thr"])
        assert 0 < sel["admitted"].size < sel["second"].size, (k, sel["admitted"].size, sel["second"].size)
        assert mo["hot_count"][k] > cap - 1 - sel["buckets"].max()  # the table leaves less room than one hash bucket
        if dtype == np.float32:
            assert mo["hot_count"][k] > 16384 and np.any((mo["code"] & 0x804000) == 0x804000)
    dev, _ = _check(oracle, mat, mo, dtype, 8, 4)
    _assert_foreign_elements(mo, dev)


@pytest.mark.parametrize("S,shift", [(16, 0), (8, 2), (32, 4)])
def test_other_maps(oracle, S, shift):
    """hub columns at other slab counts and granules; fp64 with CSR5HIP_OPT_NARROW_VALUES, so that the fp32 copy's pieces of four are seen too"""
    mat = _hub_columns_matrix(3000, 50000, 12, 300, 1)
    mo = R.build_model(mat.m, mat.n, mat.row_ptr, mat.col, S, shift, 8, HOT_LDS_BYTES // 8, MIN_COUNT)
    dev, _ = _check(oracle, mat, mo, np.float64, S, shift, narrow=1)
    _assert_foreign_elements(mo, dev)


def test_slabs_without_a_column(oracle):
    mat = empty_slabs()
    mo = _model(empty_slabs, None, 8, 4, 8)
    dev, _ = _check(oracle, mat, mo, np.float64, 8, 4)
    assert np.all(np.diff(dev["slab_off"])[:3] > 0)
    tail_word = dev["range_head"][8 * 256]
    for k in range(3, 8):
        assert dev["slab_off"][k] == dev["slab_off"][k + 1] == mat.nnz and dev["tile0"][k] == dev["tile0"][k + 1]
        assert np.all(dev["range_begin"][k] == dev["tile0"][k])
        assert np.all(dev["range_head"][k * 256:(k + 1) * 256] == tail_word)  # nothing but the CSR tail follows
    # ... and inside a slab that has tiles, every range without one carries the head of the next range that has some
    for k in range(3):
        has_tiles = np.diff(dev["range_begin"][k]) > 0
        head = dev["range_head"][k * 256:(k + 1) * 256 + 1]
        assert has_tiles.any() and not has_tiles.all()
        for rho in np.flatnonzero(~has_tiles):
            assert head[rho] == head[rho + 1]


def _digest(arrays):
    h = hashlib.sha256()
    for name in ("hot_cols", "cold_cols", "col_lo", "col_hi", "range_begin", "range_head"):
        h.update(np.ascontiguousarray(arrays[name]).tobytes())
    return h.hexdigest()


def test_structure_depends_on_the_pattern_alone(oracle, tmp_path):
    """the overfull fp64 matrix, where the second class is contested: a fresh handle, the same after asCSR / asCSR5, one loaded from save() and
    given the same options, a fresh one with other values and that one after updateValues all hold the same table columns, cold regions, codes,
    cuts and heads, and real values give the same bits of y over the non-empty rows, within 1e-12 * sum|a x| of the oracle"""
    mat = overfull_tables(22000)
    val, x = M.fill_values(mat.nnz, mat.n, np.float64, seed=9, mode="real")
    other, _ = M.fill_values(mat.nnz, mat.n, np.float64, seed=10, mode="real")
    exp = oracle.csr_spmv(mat.m, mat.row_ptr, mat.col, val, x)
    scale = oracle.csr_spmv(mat.m, mat.row_ptr, mat.col, np.abs(val), np.abs(x))
    has = np.diff(mat.row_ptr) > 0
    xd = torch.from_numpy(x).to(DEV)

    A = _handle(mat, val, xd, np.float64, 8, 4)
    assert A.info().slab_hot == 1 and A.slab_view().stride == 1
    fresh = _spmv(A, xd, mat.m, np.float64)
    assert np.all(np.abs(fresh - exp)[has] <= 1e-12 * np.maximum(scale, 1.0)[has])
    digest = _digest(A.slab_child_arrays())
    path = os.path.join(str(tmp_path), "a.csr5")
    assert A.save(path) == 0
    assert A.asCSR() == 0 and A.asCSR5() == 0, _capi.last_error()
    assert _digest(A.slab_child_arrays()) == digest, "reconverted"
    assert np.array_equal(_spmv(A, xd, mat.m, np.float64)[has], fresh[has]), "reconverted"
    assert A.destroy() == 0
    A.close()
    B = H.anonymouslibHandle.load(path)
    assert B.setColumnSlabs(8) == 0 and B.setSlabShift(4) == 0 and B.setSlabHot(2) == 0 and B.info().slab_hot == 1, _capi.last_error()
    assert _digest(B.slab_child_arrays()) == digest, "saved and loaded"
    assert np.array_equal(_spmv(B, xd, mat.m, np.float64)[has], fresh[has]), "saved and loaded"
    B.close()
    U = _handle(mat, other, xd, np.float64, 8, 4)
    assert _digest(U.slab_child_arrays()) == digest, "other values"
    assert U.updateValues(torch.from_numpy(val).to(DEV)) == 0, _capi.last_error()
    assert _digest(U.slab_child_arrays()) == digest, "update_values"
    assert np.array_equal(_spmv(U, xd, mat.m, np.float64)[has], fresh[has]), "update_values"
    assert U.destroy() == 0
    U.close()


def test_the_view_needs_a_hot_slab_child():
    """csr5hip_get_slab_view returns the invalid-argument code, with a text and without touching the struct, before conversion, without a
    table, after asCSR and on a matrix that fell back to the plain kernel; it succeeds again after a conversion that builds the table"""
    lib = _capi.load()

    def refused(A):
        view = _capi.SlabView()
        C.memset(C.byref(view), 0xAB, C.sizeof(view))
        before = bytes(view)
        assert lib.csr5hip_get_slab_view(A._h, C.byref(view)) == _capi.INVALID_ARGUMENT
        assert bytes(view) == before and "csr5hip_get_slab_view" in _capi.last_error()
        with pytest.raises(RuntimeError):
            A.slab_child_arrays()

    mat = empty_slabs()
    val, x = _int_values(mat, np.float64)
    xd = torch.from_numpy(x).to(DEV)
    rp, ci, va = _device_csr(mat, val, np.float64)
    A = H.anonymouslibHandle(mat.m, mat.n)
    assert A.inputCSR(mat.nnz, rp, ci, va) == 0 and A.setX(xd) == 0 and A.setSigma(SIGMA) == 0
    assert lib.csr5hip_get_slab_view(A._h, None) == _capi.INVALID_ARGUMENT and lib.csr5hip_get_slab_view(None, None) == _capi.INVALID_ARGUMENT
    refused(A)  # before conversion
    assert A.setColumnSlabs(8) == 0 and A.setSlabHot(0) == 0 and A.asCSR5() == 0, _capi.last_error()
    assert A.info().column_slabs == 8 and A.info().slab_hot == 0
    refused(A)  # slabs without a table
    assert A.asCSR() == 0 and A.setSlabHot(2) == 0 and A.asCSR5() == 0, _capi.last_error()
    assert A.info().slab_hot == 1 and A.slab_view().S == 8 and A.slab_child_arrays()["segments"] == A.info().slab_segments
    assert A.asCSR() == 0
    refused(A)  # after asCSR
    assert A.asCSR5() == 0 and A.slab_view().S == 8  # ... and again after reconversion
    assert A.destroy() == 0
    A.close()

    # x = 4.8 MB, scattered columns: auto picks slabs, a cap of 1 MiB makes the build fall back
    big = M.csr_from_row_lengths(np.full(60000, 10), 600000, np.random.default_rng(11), band=0.0, name="scattered")
    val, x = _int_values(big, np.float64)
    xd = torch.from_numpy(x).to(DEV)
    rp, ci, va = _device_csr(big, val, np.float64)
    F = H.anonymouslibHandle(big.m, big.n)
    assert F.inputCSR(big.nnz, rp, ci, va) == 0 and F.setX(xd) == 0 and F.setSigma(SIGMA) == 0
    assert F.setSlabMemoryMiB(1) == 0 and F.asCSR5() == 0, _capi.last_error()
    assert F.info().slab_fallback == 1 and F.info().column_slabs == 0
    refused(F)
    assert F.destroy() == 0
    F.close()
