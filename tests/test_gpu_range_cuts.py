"""The range kernel's tile ranges cut by modelled cost (csrc/csr5_range_cut.h, the table k_range_cuts makes at conversion): the persistent
hot-table kernel on matrices whose cold lanes and row starts are as uneven as they get, so that the cuts differ as much as possible from equal
tile counts -- empty ranges next to long ones, slabs with fewer tiles than ranges, a row that crosses every range of a slab.

Every case: setColumnSlabs(8), setSlabHot(2), sigma 16, fp64 and fp32, integer data, y EXACTLY the oracle's (including which rows stay
untouched).  The last test runs real values through a fresh, a reconverted, a saved-and-loaded and an update_values handle: the cuts are a function
of the pattern alone, so the four give the same bits, within 1e-12 * sum|a x| of the oracle (the bar of test_slab_hot_real_data_and_auto)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from benchmark_spmv_using_csr5_amd import _capi  # noqa: E402
from benchmark_spmv_using_csr5_amd import handle as H  # noqa: E402
from benchmark_spmv_using_csr5_amd import matrices as M  # noqa: E402
from tests.test_gpu_parity import DEV, Y_POISON, _device_csr, _expected_y, _run  # noqa: E402

SIGMA = 16


def _from_lengths(lens, cols, n, name):
    lens = np.asarray(lens, dtype=np.int64)
    row_ptr = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    assert row_ptr[-1] == cols.size
    return M.CsrMatrix(m=lens.size, n=n, row_ptr=row_ptr.astype(np.int32), col=cols.astype(np.int32), val=np.zeros(cols.size), name=name)


def hub_rows_then_short_rows():
    """(a) 2 000 rows of 300 non-zeros in 400 hub columns (each used 1 500 times: table slots), then 60 000 rows of 2 non-zeros in 300 000
    unpopular columns (each used less than once: cold).  The first tiles of every slab are all hot with few row starts, the last ones all cold
    with a row start every other element."""
    rng = np.random.default_rng(11)
    n = 300000
    hubs = rng.choice(n, size=400, replace=False)
    cols = np.concatenate([hubs[rng.integers(0, 400, size=2000 * 300)], rng.integers(0, n, size=60000 * 2)])
    return _from_lengths([300] * 2000 + [2] * 60000, cols, n, "hub_rows_then_short_rows")


def fewer_tiles_than_ranges():
    """(b) 4 096 x 4 096 with 40 000 non-zeros: 78 tiles of 512 (39 of 1 024) on 8 slabs of 256 ranges"""
    rng = np.random.default_rng(12)
    lens = rng.multinomial(40000, np.full(4096, 1 / 4096))
    return _from_lengths(lens, rng.integers(0, 4096, size=40000), 4096, "fewer_tiles_than_ranges")


def one_long_row():
    """(c) one row of 200 000 non-zeros on a sparse background: in every slab the row's segment crosses some 48 tiles and, with 256 ranges on
    those few tiles, a run of ranges longer than RUN_WAVE = 64 (most of them empty) that k_range_finish sums with a whole wavefront"""
    rng = np.random.default_rng(13)
    m, n = 20000, 250000
    lens = rng.integers(0, 4, size=m)
    lens[7001] = 200000
    return _from_lengths(lens, rng.integers(0, n, size=int(lens.sum())), n, "one_long_row")


def every_column_hot():
    """(d) 2 000 columns used 100 times each: every one gets a table slot, no lane is cold"""
    rng = np.random.default_rng(14)
    lens = rng.integers(0, 41, size=10000)
    return _from_lengths(lens, rng.integers(0, 2000, size=int(lens.sum())), 2000, "every_column_hot")


def every_column_cold():
    """(d) 200 000 non-zeros on 400 000 columns: no column is used 16 times, every lane is cold"""
    rng = np.random.default_rng(15)
    lens = rng.integers(0, 41, size=10000)
    return _from_lengths(lens, rng.integers(0, 400000, size=int(lens.sum())), 400000, "every_column_cold")


MATRICES = [hub_rows_then_short_rows, fewer_tiles_than_ranges, one_long_row, every_column_hot, every_column_cold]


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("make", MATRICES, ids=[f.__name__ for f in MATRICES])
def test_cost_cut_ranges_integer_data_bit_exact(oracle, make, dtype):
    mat = make()
    val, x = M.fill_values(mat.nnz, mat.n, dtype, seed=5, mode="int")
    if dtype == np.float32:  # (row sums stay far below 2^24: exact in fp32 too)
        val, x = (val % 3).astype(np.float32), (x % 3).astype(np.float32)
    fmt = oracle.convert(64, SIGMA, mat.m, mat.row_ptr, mat.col, val)
    info = {}
    _, _, _, ys = _run(mat, val, x, SIGMA, H.SPMV_FUSED, dtype=dtype, slabs=8, hot=2, repeat=2, info_out=info)
    assert info["slab_hot"] == 1 and info["column_slabs"] == 8, info
    if make is every_column_hot:
        assert info["slab_hot_cover_pct"] >= 99, info
    if make is every_column_cold:
        assert info["slab_hot_cover_pct"] == 0, info
    exp = _expected_y(oracle, fmt, mat, x, Y_POISON)
    for y in ys:
        assert np.array_equal(y, exp), (mat.name, np.flatnonzero(y != exp)[:8])


def _spmv(A, x, m):
    y = torch.full((m,), Y_POISON, dtype=torch.float64, device=DEV)
    assert A.setX(x) == 0 and A.spmv(1.0, y) == 0, _capi.last_error()
    torch.cuda.synchronize()
    return y.cpu().numpy()


def test_same_bits_from_fresh_reconverted_loaded_and_updated_handles(oracle, tmp_path):
    """Real values on matrix (a) plus a long row: a row that straddles a range boundary is added in an association the cuts fix, and the cuts
    come from the pattern alone."""
    base = hub_rows_then_short_rows()
    rng = np.random.default_rng(16)
    lens = np.diff(base.row_ptr).astype(np.int64)
    extra = rng.integers(0, base.n, size=30000)
    cols = np.concatenate([base.col[:base.row_ptr[1000]], extra, base.col[base.row_ptr[1000]:]])
    lens[999] += 30000
    mat = _from_lengths(lens, cols, base.n, "hub_rows_long_row")
    val, x = M.fill_values(mat.nnz, mat.n, np.float64, seed=9, mode="real")
    other, _ = M.fill_values(mat.nnz, mat.n, np.float64, seed=10, mode="real")
    exp = oracle.csr_spmv(mat.m, mat.row_ptr, mat.col, val, x)
    scale = oracle.csr_spmv(mat.m, mat.row_ptr, mat.col, np.abs(val), np.abs(x))
    has = np.diff(mat.row_ptr) > 0
    xd = torch.from_numpy(x).to(DEV)

    def handle(values):
        rp, ci, va = _device_csr(mat, values, np.float64)
        A = H.anonymouslibHandle(mat.m, mat.n)
        assert A.inputCSR(mat.nnz, rp, ci, va) == 0 and A.setX(xd) == 0 and A.setSigma(SIGMA) == 0
        assert A.setColumnSlabs(8) == 0 and A.setSlabHot(2) == 0 and A.asCSR5() == 0, _capi.last_error()
        assert A.info().slab_hot == 1
        return A

    A = handle(val)
    fresh = _spmv(A, xd, mat.m)
    assert np.array_equal(fresh[has], _spmv(A, xd, mat.m)[has]), "run to run"
    assert np.all(np.abs(fresh - exp)[has] <= 1e-12 * np.maximum(scale, 1.0)[has])
    path = os.path.join(str(tmp_path), "a.csr5")
    assert A.save(path) == 0
    assert A.asCSR() == 0 and A.asCSR5() == 0, _capi.last_error()
    assert np.array_equal(_spmv(A, xd, mat.m)[has], fresh[has]), "reconverted"
    assert A.destroy() == 0
    A.close()
    B = H.anonymouslibHandle.load(path)
    assert B.setColumnSlabs(8) == 0 and B.setSlabHot(2) == 0 and B.info().slab_hot == 1, _capi.last_error()
    assert np.array_equal(_spmv(B, xd, mat.m)[has], fresh[has]), "saved and loaded"
    B.close()
    U = handle(other)
    assert U.updateValues(torch.from_numpy(val).to(DEV)) == 0, _capi.last_error()
    assert np.array_equal(_spmv(U, xd, mat.m)[has], fresh[has]), "update_values"
    assert U.destroy() == 0
    U.close()
