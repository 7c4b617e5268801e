"""The definition of csr5hip_spmm_reduce and its gradients (include/csr5hip_reduce.h) in numpy, oracle-independent.

* ``forward``  t(e, c) = val[e] * X[col(e), c] (one multiplication in the working precision) or X[col(e), c]; per row and column the
  winner under the contract's total order: the first NaN if the column of the row holds one, otherwise the first occurrence -- the
  smallest rank -- of the row's largest +t (max) or -t (min), +0 == -0 ties included (segment reductions over the rows with
  entries: ``maximum.reduceat`` for the value, ``minimum.reduceat`` over the ranks that attain it).  Y = t[arg] bit for bit; a row
  without entries gets +0 and -1.  (An ``argmax`` over ``where(isnan(t), +inf, t)`` would let a +Inf of smaller rank tie with a NaN;
  the order says the NaN wins, so NaN columns are decided first.)
* ``dval``     the chain acc = fma(X[col(e), c], dY[i, c], acc) from +0 over the c with arg[i, c] == e in ascending c, by the C
  library's correctly rounded ``fma`` / ``fmaf``.  An arg outside its row's rank range matches no entry.
* ``dx``       in float64: the sum of the winning terms per (j, c), with the number of winning terms w and the sum of their
  magnitudes, from which the bound |got - ref| <= (w + 1) u sum|a_e dY| follows: one rounding per product and w - 1 additions
  (w with the +0 the chains start from), each at most u times the running magnitude (Higham, section 4.2, first order).
"""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype, _libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3
_libm.fmaf.restype, _libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3


def fma(a, b, c, dtype):
    """a * b + c with one rounding, in `dtype`"""
    if np.dtype(dtype) == np.float64:
        return np.float64(_libm.fma(float(a), float(b), float(c)))
    return np.float32(_libm.fmaf(float(a), float(b), float(c)))


def rows_of(mat) -> np.ndarray:
    return np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr).astype(np.int64))


def terms(mat, val, X, weighted=True) -> np.ndarray:
    """t (nnz, k) in X's dtype"""
    cols = np.asarray(mat.col[:mat.nnz], dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(val, dtype=X.dtype)[:, None] * X[cols]) if weighted else X[cols].copy()


def forward(mat, val, X, op="max", weighted=True):
    """(Y (m, k) of X's dtype, arg (m, k) int32)"""
    t = terms(mat, val, X, weighted)
    k = X.shape[1]
    Y = np.zeros((mat.m, k), dtype=X.dtype)
    arg = np.full((mat.m, k), -1, dtype=np.int32)
    has = np.flatnonzero(np.diff(mat.row_ptr) > 0)
    if k == 0 or has.size == 0:
        return Y, arg
    # the rows with entries tile 0 .. nnz: reduceat over their starts reduces exactly each row
    starts = mat.row_ptr[:-1].astype(np.int64)[has]
    local = np.repeat(np.arange(has.size), np.diff(mat.row_ptr).astype(np.int64)[has])
    rank = np.arange(mat.nnz, dtype=np.int64)[:, None]
    nan = np.isnan(t)
    key = np.where(nan, -np.inf, t if op == "max" else -t)
    best = np.maximum.reduceat(key, starts, axis=0)                                        # the winning value, NaN aside
    first = np.minimum.reduceat(np.where(key == best[local], rank, mat.nnz), starts, axis=0)  # its first occurrence: the smallest rank
    first_nan = np.minimum.reduceat(np.where(nan, rank, mat.nnz), starts, axis=0)
    win = np.where(first_nan < mat.nnz, first_nan, first)                                  # a NaN beats every number
    arg[has] = win
    Y[has] = t[win, np.arange(k)[None, :]]
    return Y, arg


def dval(mat, X, dY, arg) -> np.ndarray:
    """(nnz,) of X's dtype"""
    dt = X.dtype
    out = np.zeros(mat.nnz, dtype=dt)
    cols = np.asarray(mat.col[:mat.nnz], dtype=np.int64)
    lo, hi = mat.row_ptr[:-1].astype(np.int64)[:, None], mat.row_ptr[1:].astype(np.int64)[:, None]
    a64 = arg.astype(np.int64)
    ii, cc = np.nonzero((a64 >= lo) & (a64 < hi))  # row-major: ascending c within a row, and an entry belongs to one row
    for i, c in zip(ii.tolist(), cc.tolist()):
        e = int(a64[i, c])
        out[e] = fma(X[cols[e], c], dY[i, c], out[e], dt)
    return out


def dx(mat, val, dY, arg, weighted=True):
    """(dX (n, k) float64, winners (n, k) int64, magnitude (n, k) float64)"""
    k = dY.shape[1]
    rows, cols = rows_of(mat), np.asarray(mat.col[:mat.nnz], dtype=np.int64)
    ranks = np.arange(mat.nnz, dtype=np.int64)
    wins = arg.astype(np.int64)[rows] == ranks[:, None]                                   # (nnz, k)
    g = dY.astype(np.float64)[rows]
    p = (np.asarray(val, dtype=np.float64)[:, None] * g) if weighted else g
    p = np.where(wins, p, 0.0)
    out, w, mag = np.zeros((mat.n, k)), np.zeros((mat.n, k), dtype=np.int64), np.zeros((mat.n, k))
    np.add.at(out, cols, p)
    np.add.at(w, cols, wins.astype(np.int64))
    np.add.at(mag, cols, np.abs(p))
    return out, w, mag


def dx_bound(w, mag, dtype) -> np.ndarray:
    u = float(np.finfo(dtype).eps) / 2
    return (w + 1) * u * mag


def same_bits(got, want) -> bool:
    """bit for bit, sign of zero included; NaN positions as positions"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    word = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.array_equal(np.isnan(got), nan)) and np.array_equal(got.view(word)[~nan], want.view(word)[~nan])


def distinct_values(nnz: int, dtype, seed: int = 11) -> np.ndarray:
    """a permutation of nnz equidistant values in [-2, 2) without a zero, distinct also in fp32"""
    v = ((np.random.default_rng(seed).permutation(nnz) + 0.5) / max(nnz, 1) * 4 - 2).astype(dtype)
    assert len(np.unique(v)) == nnz
    return v
