"""Oracle-independent reference for the sampled dense-dense product out[e] = dot(U[row(e), :], V[col(e), :]) on the pattern of
any ``CsrMatrix`` (pure numpy and ``math``), in the manner of tests/exact_reference.py.

Five datasets of (U, V), U (m, k) and V (n, k), for fp64 and fp32:

* ``integer``     small integers: every dot product is exact in any order.
* ``row_scaled``  small integers times 2**r per row of U and per row of V, r over +-400 (fp64) / +-40 (fp32): all k products
  of an element share one power of two, so its sum stays exact and representable, while neighbouring elements of a tile
  differ by hundreds of orders of magnitude.
* ``subnormal``   per column c either U[:, c] or V[:, c] carries 2**-1060 (fp64) / 2**-140 (fp32): every product is an integer
  multiple of it, the sums are subnormal and exact; any flush fails.
* ``nonfinite``   integers 0..9 (zeros included, so 0 * Inf = NaN occurs) with +Inf, -Inf or NaN in a few rows of U and of V,
  row 0 of each always.  An element whose two rows are finite must come out exact whatever its neighbours hold.
* ``wide_range``  +-(26-bit int) * 2**e for fp64, +-(12-bit int) * 2**e for fp32: every product is exact in the working
  precision, the sum is not.

The reference of an element (``reference``):

* exact datasets: NaN if any of its k products is NaN or products of both +Inf and -Inf occur, else +-Inf if any product is
  infinite, else the exact sum.  (The finite products of these datasets are small-integer multiples of one power of two per
  element: every partial sum is exact in float64, so numpy's row sum IS the exact sum; it is asserted representable in the
  working precision.)  Compared by value, NaN matching NaN.
* ``wide_range``: s = ``math.fsum`` of the products and |out - s| <= gamma(k) * sum|product| + u |s|, gamma(k) = k u / (1 - k u),
  u the unit roundoff.  Derivation: any summation tree over k exact products, with or without FMA, performs at most k roundings
  on the path of a product to the root, so the computed value is sum p_i (1 + theta_i) with |theta_i| <= gamma(k) (Higham,
  Accuracy and Stability of Numerical Algorithms, section 4.2); u |s| covers the comparison against the rounded s.  No
  absolute floor.

Every element is checked; k = 0 expects +0.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests.exact_reference import unit_roundoff

DATASETS = ("integer", "row_scaled", "subnormal", "nonfinite", "wide_range")
DTYPES = (np.float64, np.float32)
SUBNORMAL_EXP = {np.float64: -1060, np.float32: -140}
ROW_SCALE_SPAN = {np.float64: 400, np.float32: 40}


def _key(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def rows_of(mat) -> np.ndarray:
    """row index of every stored element, CSR order"""
    return np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr).astype(np.int64))


def make(dataset: str, mat, k: int, dtype, seed: int = 0):
    """(U, V): U (m, k) and V (n, k) of `dtype`, C-contiguous"""
    dt = _key(dtype)
    rng = np.random.default_rng([seed, DATASETS.index(dataset), 64 if dt == np.float64 else 32, k])
    m, n = mat.m, mat.n
    if dataset == "integer":
        U = rng.integers(-4, 6, size=(m, k)).astype(dt)
        V = rng.integers(-4, 6, size=(n, k)).astype(dt)
    elif dataset == "row_scaled":
        hi = 10 if dt == np.float64 else 3
        span = ROW_SCALE_SPAN[dt]
        ru = rng.integers(-span, span + 1, size=(m, 1))
        rv = rng.integers(-span, span + 1, size=(n, 1))
        U = np.ldexp(rng.integers(0, hi, size=(m, k)).astype(np.float64), ru).astype(dt)
        V = np.ldexp(rng.integers(0, hi, size=(n, k)).astype(np.float64), rv).astype(dt)
    elif dataset == "subnormal":
        e = SUBNORMAL_EXP[dt]
        on_u = rng.random(k) < 0.5  # columns whose 2**e sits on U
        U = np.ldexp(rng.integers(0, 10, size=(m, k)).astype(np.float64), np.where(on_u, e, 0)[None, :]).astype(dt)
        V = np.ldexp(rng.integers(0, 10, size=(n, k)).astype(np.float64), np.where(on_u, 0, e)[None, :]).astype(dt)
    elif dataset == "nonfinite":
        U = rng.integers(0, 10, size=(m, k)).astype(dt)
        V = rng.integers(0, 10, size=(n, k)).astype(dt)
        specials = np.array([np.inf, -np.inf, np.nan], dtype=dt)
        for W, rows in ((U, m), (V, n)):
            if rows and k:
                bad = np.unique(np.concatenate([[0], rng.choice(rows, size=min(rows, 2 + rows // 400), replace=False)]))
                for r in bad.tolist():
                    cols = rng.choice(k, size=1 + int(rng.integers(0, min(k, 3))), replace=False)
                    W[r, cols] = specials[rng.integers(0, 3, size=cols.size)]
    elif dataset == "wide_range":
        bits, span = (26, 200) if dt == np.float64 else (12, 30)

        def draw(shape):
            mant = rng.integers(1, 2 ** bits, size=shape).astype(np.float64) * rng.choice([-1.0, 1.0], size=shape)
            return np.ldexp(mant, rng.integers(-span, span + 1, size=shape))
        U, V = draw((m, k)).astype(dt), draw((n, k)).astype(dt)
    else:
        raise ValueError(dataset)
    return np.ascontiguousarray(U), np.ascontiguousarray(V)


@dataclass
class Reference:
    dtype: type
    expected: np.ndarray   # float64 (nnz,): the exact value, or fsum of the products (bounded elements)
    bound: np.ndarray      # float64 (nnz,): < 0 = compared exactly, else the allowed |out - expected|


def reference(dataset: str, mat, U, V) -> Reference:
    dt = _key(U.dtype)
    u = unit_roundoff(dt)
    k = U.shape[1]
    nnz = mat.nnz
    rows, cols = rows_of(mat), np.asarray(mat.col[:nnz], dtype=np.int64)
    with np.errstate(invalid="ignore"):  # 0 * Inf = NaN is part of the data
        P = U.astype(np.float64)[rows] * V.astype(np.float64)[cols]  # (nnz, k); exact: no product rounds in any dataset
    if dt == np.float32:
        assert np.array_equal(P.astype(np.float32).astype(np.float64), P, equal_nan=True), "a product is not exact in fp32"
    expected = np.zeros(nnz, dtype=np.float64)
    bound = np.full(nnz, -1.0)
    if k == 0 or nnz == 0:
        return Reference(dt, expected, bound)
    if dataset == "wide_range":
        assert np.isfinite(P).all()
        g = k * u / (1.0 - k * u)
        pl, al = P.tolist(), np.abs(P).tolist()
        for e in range(nnz):
            s = math.fsum(pl[e])
            expected[e] = s
            # (1 + 2**-50): the rounding of this bound's own float64 evaluation and of |out - s| in bad_elements
            bound[e] = (g * math.fsum(al[e]) + u * abs(s)) * (1.0 + 2.0 ** -50)
        return Reference(dt, expected, bound)
    nan = np.isnan(P).any(axis=1) | (np.isposinf(P).any(axis=1) & np.isneginf(P).any(axis=1))
    posinf, neginf = np.isposinf(P).any(axis=1) & ~nan, np.isneginf(P).any(axis=1) & ~nan
    finite = ~(nan | posinf | neginf)
    s = np.where(finite[:, None], P, 0.0).sum(axis=1)  # exact (see the module docstring)
    assert np.array_equal(s.astype(dt).astype(np.float64), s), "an exact sum is not representable"  # generator invariant
    expected[:] = s
    expected[nan], expected[posinf], expected[neginf] = np.nan, np.inf, -np.inf
    return Reference(dt, expected, bound)


def bad_elements(out, ref: Reference) -> np.ndarray:
    out = np.asarray(out)
    assert out.dtype == ref.dtype and out.shape == ref.expected.shape, (out.dtype, out.shape, ref.expected.shape)
    od, e = out.astype(np.float64), ref.expected
    with np.errstate(invalid="ignore"):
        exact_ok = (od == e) | (np.isnan(od) & np.isnan(e))
        bound_ok = np.abs(od - e) <= ref.bound
    return np.flatnonzero(~np.where(ref.bound < 0, exact_ok, bound_ok))


def check(out, ref: Reference, what="") -> None:
    bad = bad_elements(out, ref)
    if bad.size:
        i = bad[:6]
        raise AssertionError(f"{what}: {bad.size} of {np.asarray(out).size} elements wrong; elements {i.tolist()}: got "
                             f"{np.asarray(out)[i].tolist()}, expected {ref.expected[i].tolist()} (bound {ref.bound[i].tolist()})")


def duplicates_matrix(seed: int = 31):
    """a matrix with repeated (row, column) pairs, empty rows and about 600 stored elements (p >= 2 at sigma 4)"""
    from benchmark_spmv_using_csr5_amd import matrices as M
    rng = np.random.default_rng(seed)
    m, n = 110, 70
    lens = rng.integers(0, 14, size=m) * (rng.random(m) < 0.8)
    lens[5] = 40
    row_ptr = np.zeros(m + 1, dtype=np.int32)
    np.cumsum(lens, out=row_ptr[1:])
    col = np.concatenate([np.sort(rng.integers(0, n, size=int(c))) for c in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    col[row_ptr[5] + 1] = col[row_ptr[5]]  # (at least one repeated pair, whatever the draw)
    assert any(np.unique(col[row_ptr[r]:row_ptr[r + 1]]).size < lens[r] for r in range(m))
    return M.CsrMatrix(m, n, row_ptr, col, np.ones(col.size, dtype=np.float64), "duplicates")
