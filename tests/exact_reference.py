"""Oracle-independent reference for y = A x on data where SpMV kernels go wrong (pure numpy and ``math``).

Four datasets, for fp64 and fp32, on the structure of any ``CsrMatrix``:

* ``row_scaled``  small integers times 2**r_i per row (r_i over about +-900 for fp64, +-100 for fp32): every row sum is
  exact, and neighbouring rows of one tile differ by up to 2**1800.  A prefix-difference segmented sum
  (``prefix[end] - prefix[start]``) returns garbage for the small rows.
* ``nonfinite``   the reference CLI's ``rand() % 10`` data (stored zeros included, so 0 * Inf = NaN happens), with a few
  x entries -- column 0 always -- set to +Inf, -Inf or NaN and a few matrix values set to Inf or NaN.  A masked lane
  computed as ``0 * x[clamped column]`` instead of a select poisons rows that never reference that column.
* ``subnormal``   products that are integer multiples of 2**-1060 (fp64) or 2**-140 (fp32): subnormal x entries, and
  subnormal matrix values in the few columns whose x entry is a plain integer.  Sums stay exact; any flush fails.
* ``wide_range``  +-(26-bit int) * 2**e for fp64, +-(12-bit int) * 2**e for fp32, e spread over about +-200 / +-30 on
  A and x: every product is exact in the working precision.  Checked against ``math.fsum`` with a bound that holds for
  ANY summation tree and has no absolute floor.

The reference of a row (``reference``):

* exact datasets: NaN if any product is NaN or products of both +Inf and -Inf occur, else +-Inf if any product is
  infinite, else the exact sum (``math.fsum`` of products that are exact, rounded once; the generators keep that sum
  representable).  Compared by value, NaN matching NaN.
* ``wide_range``: s = fsum of the products, and |y - s| <= gamma(n_i - 1) * sum|p| + 2**-53 |s| with
  gamma(k) = k u / (1 - k u), u the unit roundoff of the working precision.  Rows of one or two entries are bit-exact.

Rows without entries follow the library's contract: below ``tail_partition_start`` they keep y0, at or above it they
are 0; with CSR5HIP_OPT_ZERO_EMPTY_ROWS every empty row is 0.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

DATASETS = ("row_scaled", "nonfinite", "subnormal", "wide_range")
DTYPES = (np.float64, np.float32)

# exponent of the products of the subnormal dataset: 2**-1060 (fp64 subnormals start below 2**-1022, step 2**-1074),
# 2**-140 (fp32: below 2**-126, step 2**-149)
SUBNORMAL_EXP = {np.float64: -1060, np.float32: -140}


def _key(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def unit_roundoff(dtype) -> float:
    return 2.0 ** -53 if _key(dtype) == np.float64 else 2.0 ** -24


def _rows(mat) -> np.ndarray:
    return np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr).astype(np.int64))


def make(dataset: str, mat, dtype, seed: int = 0, k: int = 1, finite_matrix: bool = False):
    """(val, X): matrix values (nnz,) and k vectors X (n, k) of `dtype`.  The columns of X are independent draws of the
    dataset's x for the same matrix values; in ``nonfinite`` only column 0 holds non-finite entries (so the other
    columns of an SpMM must come out exact), and ``finite_matrix`` keeps every matrix value finite."""
    dt = _key(dtype)
    rng = np.random.default_rng([seed, DATASETS.index(dataset), 64 if dt == np.float64 else 32])
    nnz, n = mat.nnz, mat.n
    rows = _rows(mat)
    X = np.empty((n, k), dtype=dt)
    if dataset == "row_scaled":
        hi, span = (10, 900) if dt == np.float64 else (3, 100)
        r = rng.integers(-span, span + 1, size=mat.m)
        val = np.ldexp(rng.integers(0, hi, size=nnz).astype(np.float64), r[rows]).astype(dt)
        for c in range(k):
            X[:, c] = rng.integers(0, hi, size=n)
    elif dataset == "nonfinite":
        val = rng.integers(0, 10, size=nnz).astype(dt)
        for c in range(k):
            X[:, c] = rng.integers(0, 10, size=n)
        if n:
            specials = np.array([np.inf, -np.inf, np.nan], dtype=dt)
            bad = np.unique(np.concatenate([[0], rng.choice(n, size=min(n, 2 + n // 600), replace=False)]))
            X[bad, 0] = specials[rng.integers(0, 3, size=bad.size)]
            X[0, 0] = specials[seed % 3]
        if nnz and not finite_matrix:
            pos = rng.choice(nnz, size=min(nnz, 1 + nnz // 2000), replace=False)
            val[pos] = np.array([np.inf, np.nan], dtype=dt)[rng.integers(0, 2, size=pos.size)]
    elif dataset == "subnormal":
        e = SUBNORMAL_EXP[dt]
        plain = rng.random(n) < 0.1  # columns whose x is a plain integer: their matrix values carry the 2**e
        a = rng.integers(0, 10, size=nnz).astype(np.float64)
        val = np.where(plain[mat.col], np.ldexp(a, e), a).astype(dt)
        for c in range(k):
            xi = rng.integers(0, 10, size=n).astype(np.float64)
            X[:, c] = np.where(plain, xi, np.ldexp(xi, e))
    elif dataset == "wide_range":
        bits, span = (26, 200) if dt == np.float64 else (12, 30)

        def draw(size):
            mant = rng.integers(1, 2 ** bits, size=size).astype(np.float64) * rng.choice([-1.0, 1.0], size=size)
            return np.ldexp(mant, rng.integers(-span, span + 1, size=size))
        val = draw(nnz).astype(dt)
        for c in range(k):
            X[:, c] = draw(n)
    else:
        raise ValueError(dataset)
    return val, X


@dataclass
class Reference:
    """What every row of y must be (see the module docstring)."""

    dtype: type
    nonempty: np.ndarray   # bool (m,): the row owns at least one entry
    expected: np.ndarray   # float64 (m,): the exact value (exact rows) or fsum of the products (bounded rows)
    bound: np.ndarray      # float64 (m,): < 0 = the row is compared exactly, else the allowed |y - expected|


def reference(dataset: str, mat, val, x) -> Reference:
    """The reference of y = A x for one vector x of `dataset`'s kind."""
    dt = _key(val.dtype)
    u = unit_roundoff(dt)
    rp = mat.row_ptr.astype(np.int64)
    lens = np.diff(rp)
    with np.errstate(invalid="ignore"):  # 0 * Inf = NaN is part of the data
        p = val.astype(np.float64) * np.asarray(x, dtype=np.float64)[mat.col]  # exact: no product rounds in any dataset
    if dt == np.float32:
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p, equal_nan=True), "a product is not exact in fp32"
    rows = _rows(mat)

    def any_per_row(flags):
        return np.bincount(rows[flags], minlength=mat.m) > 0

    nan = any_per_row(np.isnan(p)) | (any_per_row(np.isposinf(p)) & any_per_row(np.isneginf(p)))
    posinf, neginf = any_per_row(np.isposinf(p)) & ~nan, any_per_row(np.isneginf(p)) & ~nan
    expected = np.zeros(mat.m, dtype=np.float64)
    bound = np.full(mat.m, -1.0)
    bounded = dataset == "wide_range"
    assert not (bounded and (nan | posinf | neginf).any())
    pl, al = p.tolist(), np.abs(p).tolist()
    for i in np.flatnonzero((lens > 0) & ~nan & ~posinf & ~neginf).tolist():
        s = math.fsum(pl[rp[i]:rp[i + 1]])
        expected[i] = s
        if bounded:
            g = (lens[i] - 1) * u / (1.0 - (lens[i] - 1) * u)
            # (1 + 2**-50): the rounding of this bound's own float64 evaluation and of |y - s| in bad_rows
            bound[i] = (g * math.fsum(al[rp[i]:rp[i + 1]]) + 2.0 ** -53 * abs(s)) * (1.0 + 2.0 ** -50)
        else:
            assert float(dt(s)) == s, f"row {i}: the exact sum {s!r} is not representable"  # generator invariant
    expected[nan] = np.nan
    expected[posinf] = np.inf
    expected[neginf] = -np.inf
    return Reference(dt, lens > 0, expected, bound)


def empty_zero_rows(m: int, tail_partition_start: int, zero_empty: bool = False) -> np.ndarray:
    """rows that an SpMV sets to 0 when they own no entry: all of them with ZERO_EMPTY_ROWS, else rows >= the tail"""
    z = np.zeros(m, dtype=bool)
    z[0 if zero_empty else max(int(tail_partition_start), 0):] = True
    return z


def bad_rows(y, ref: Reference, zero_rows: np.ndarray, y0) -> np.ndarray:
    """indices of the rows of y that break the reference (empty rows: 0 where `zero_rows`, else y0 bit for bit)"""
    y = np.asarray(y)
    assert y.dtype == ref.dtype and y.shape == ref.expected.shape, (y.dtype, y.shape)
    yd = y.astype(np.float64)
    e = ref.expected
    with np.errstate(invalid="ignore"):
        exact_ok = (yd == e) | (np.isnan(yd) & np.isnan(e))
        bound_ok = np.abs(yd - e) <= ref.bound
    ok = np.where(ref.bound < 0, exact_ok, bound_ok)
    poison = np.full(1, y0, dtype=ref.dtype).view(np.uint64 if ref.dtype == np.float64 else np.uint32)[0]
    bits = y.view(np.uint64 if ref.dtype == np.float64 else np.uint32)
    empty_ok = np.where(zero_rows, yd == 0.0, bits == poison)
    return np.flatnonzero(~np.where(ref.nonempty, ok, empty_ok))


def check(y, ref: Reference, zero_rows: np.ndarray, y0, what="") -> None:
    bad = bad_rows(y, ref, zero_rows, y0)
    if bad.size:
        i = bad[:6]
        raise AssertionError(f"{what}: {bad.size} of {y.size} rows wrong; rows {i.tolist()}: got {np.asarray(y)[i].tolist()}, "
                             f"expected {ref.expected[i].tolist()} (bound {ref.bound[i].tolist()}, "
                             f"nonempty {ref.nonempty[i].tolist()})")
