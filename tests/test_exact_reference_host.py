"""The exact reference of tests/exact_reference.py, on the host (no GPU).

1. The CPU oracle's CSR5 SpMV passes all four datasets on the zoo at sigma 4, 7, 16 and 32: the reference's semantics
   (non-finite rules, empty rows, bounds) are right before any GPU kernel is held to them.
2. The checker has teeth: four numpy restatements of kernel bugs that the integer and uniform(-1, 1) checks of the older
   suite cannot see are each rejected on the dataset built for them.
"""
import numpy as np
import pytest

from tests import exact_reference as R
from tests import zoo

SIGMAS = (4, 7, 16, 32)
Y0 = 777.0


def _dt(dtype):
    return "fp64" if dtype == np.float64 else "fp32"


def _rows(mat):
    return np.repeat(np.arange(mat.m), np.diff(mat.row_ptr))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("dataset", R.DATASETS)
def test_oracle_passes_every_dataset(oracle, dataset, dtype):
    for mat in zoo.small_zoo():
        val, X = R.make(dataset, mat, dtype, seed=3)
        x = X[:, 0]
        ref = R.reference(dataset, mat, val, x)
        assert ref.nonempty.any()
        for sigma in SIGMAS:
            fmt = oracle.convert(64, sigma, mat.m, mat.row_ptr, mat.col, val)
            with np.errstate(invalid="ignore", over="ignore"):
                y = oracle.spmv(fmt, mat.row_ptr, x, y0=np.full(mat.m, Y0, dtype=dtype))
            R.check(y, ref, R.empty_zero_rows(mat.m, fmt.tail_start), Y0, f"oracle {mat.name} {dataset} sigma {sigma}")


def test_datasets_are_what_they_claim():
    """x[0] is non-finite and stored zeros meet infinities; subnormal data really is subnormal; fp64 rows of row_scaled
    span 2**+-900; wide_range's products are exact."""
    mat = zoo.small_zoo()[5]
    for dtype in R.DTYPES:
        val, X = R.make("nonfinite", mat, dtype, seed=1)
        assert not np.isfinite(X[0, 0]) and np.isinf(X[:, 0]).any() and np.isnan(X[:, 0]).any()
        assert (~np.isfinite(val)).any() and (val == 0).any()
        val, X = R.make("subnormal", mat, dtype, seed=1)
        tiny = np.finfo(dtype).tiny
        assert ((np.abs(X) < tiny) & (X != 0)).mean() > 0.5 and ((np.abs(val) < tiny) & (val != 0)).any()
        val, X = R.make("wide_range", mat, dtype, seed=1)
        e = np.frexp(val)[1]
        assert e.max() - e.min() > (300 if dtype == np.float64 else 50)
    val, _ = R.make("row_scaled", mat, np.float64, seed=1)
    e = np.frexp(val[val != 0])[1]
    assert e.min() < -800 and e.max() > 800


# ---- mutants ---------------------------------------------------------------------------------------------------------

def _correct(mat, val, x, tail_start, y0, dtype, products=None):
    """a right answer computed a plain way (float64 accumulation of exact products), with the empty-row contract"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = val.astype(np.float64) * x.astype(np.float64)[mat.col] if products is None else products
        y = np.zeros(mat.m, dtype=np.float64)
        np.add.at(y, _rows(mat), p)
    return _contract(mat, y.astype(dtype), tail_start, y0)


def _contract(mat, y, tail_start, y0):
    empty = np.diff(mat.row_ptr) == 0
    y = y.copy()
    y[empty & (np.arange(mat.m) < tail_start)] = y0
    y[empty & (np.arange(mat.m) >= tail_start)] = 0
    return y


def _prefix_difference(mat, val, x, sigma, tail_start, y0, dtype):
    """mutant (a): per tile of 64 * sigma entries, a running sum over the tile's stream, each row segment taken as
    prefix[end] - prefix[start - 1] (the shape of a shuffle-scan segmented sum that subtracts scan results)"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = (val * x[mat.col]).astype(dtype)
        rows = _rows(mat)
        y = np.zeros(mat.m, dtype=dtype)
        T = 64 * sigma
        for t0 in range(0, mat.nnz, T):
            P = np.cumsum(p[t0:t0 + T], dtype=dtype)
            r = rows[t0:t0 + T]
            starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
            ends = np.r_[starts[1:], r.size]
            before = np.where(starts > 0, P[np.maximum(starts - 1, 0)], dtype(0))
            np.add.at(y, r[starts], P[ends - 1] - before)
    return _contract(mat, y, tail_start, y0)


def _rejected(dataset, dtype, mutant, sigma=4):
    """the matrices of the zoo on which the checker rejects `mutant`, and the number it was tried on"""
    from oracle.csr5_oracle import Oracle
    orc = Oracle()
    rejected, tried = [], 0
    for mat in zoo.small_zoo():
        val, X = R.make(dataset, mat, dtype, seed=3)
        x = X[:, 0]
        ref = R.reference(dataset, mat, val, x)
        tail = orc.convert(64, sigma, mat.m, mat.row_ptr, mat.col, val).tail_start
        y = mutant(mat, val, x, sigma, tail, Y0, dtype)
        # the plain right answer passes the same check: the rejection is the mutant's doing
        R.check(_correct(mat, val, x, tail, Y0, dtype), ref, R.empty_zero_rows(mat.m, tail), Y0, f"control {mat.name}")
        tried += 1
        if R.bad_rows(y, ref, R.empty_zero_rows(mat.m, tail), Y0).size:
            rejected.append(mat.name)
    return rejected, tried


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
@pytest.mark.parametrize("dataset", ["row_scaled", "nonfinite"])
def test_mutant_prefix_difference_rejected(dataset, dtype):
    rejected, tried = _rejected(dataset, dtype, _prefix_difference)
    # most zoo matrices hold, in one tile, a small row behind a large one (or behind an infinity)
    assert len(rejected) >= 2 * tried // 3, (rejected, tried)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_mutant_masked_lane_times_x0_rejected(dtype):
    """mutant (b): 0 * x[0] added to every written row (a masked lane that multiplies instead of selecting)"""
    def mutant(mat, val, x, sigma, tail, y0, dtype):
        y = _correct(mat, val, x, tail, y0, dtype)
        written = (np.diff(mat.row_ptr) > 0) | (np.arange(mat.m) >= tail)
        with np.errstate(invalid="ignore"):
            y[written] += dtype(0) * x[0]
        return y
    rejected, tried = _rejected("nonfinite", dtype, mutant)
    # (a matrix whose every row already references a non-finite entry cannot tell)
    assert len(rejected) >= tried - 2, (rejected, tried)


def test_mutant_fp32_accumulation_rejected():
    """mutant (c): fp64 rows accumulated in fp32"""
    def mutant(mat, val, x, sigma, tail, y0, dtype):
        with np.errstate(invalid="ignore", over="ignore"):
            p = val.astype(np.float32) * x.astype(np.float32)[mat.col]
            y = np.zeros(mat.m, dtype=np.float32)
            np.add.at(y, _rows(mat), p)
        return _contract(mat, y.astype(np.float64), tail, y0)
    rejected, tried = _rejected("wide_range", np.float64, mutant)
    assert len(rejected) == tried, (rejected, tried)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_dt)
def test_mutant_subnormal_flush_rejected(dtype):
    """mutant (d): products below the smallest normal number flushed to zero"""
    def mutant(mat, val, x, sigma, tail, y0, dtype):
        p = val.astype(np.float64) * x.astype(np.float64)[mat.col]
        p[np.abs(p) < np.finfo(dtype).tiny] = 0.0
        return _correct(mat, val, x, tail, y0, dtype, products=p)
    rejected, tried = _rejected("subnormal", dtype, mutant)
    assert len(rejected) == tried, (rejected, tried)


def test_checker_rejects_one_ulp_and_a_touched_empty_row():
    """single-entry rows of wide_range are bit-exact (one ulp off fails); an empty row below the tail must keep y0 bit for
    bit, one at or above it must be 0"""
    mat = zoo.kat0()
    for dtype in R.DTYPES:
        val, X = R.make("wide_range", mat, dtype, seed=2)
        x = X[:, 0]
        ref = R.reference("wide_range", mat, val, x)
        tail = 4
        y = _correct(mat, val, x, tail, Y0, dtype)
        zr = R.empty_zero_rows(mat.m, tail)
        R.check(y, ref, zr, Y0, "exact")
        one = np.flatnonzero(np.diff(mat.row_ptr) == 1)[0]
        bumped = y.copy()
        bumped[one] = np.nextafter(bumped[one], dtype(np.inf))
        assert R.bad_rows(bumped, ref, zr, Y0).tolist() == [one]
        touched = y.copy()
        touched[1] = 0  # row 1 is empty and below the tail
        assert R.bad_rows(touched, ref, zr, Y0).tolist() == [1]
        assert R.bad_rows(y, ref, R.empty_zero_rows(mat.m, tail, zero_empty=True), Y0).tolist() == [1]
