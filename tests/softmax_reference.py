"""Oracle-independent reference for the softmax over the stored entries of every row and for its gradient (csr5hip_row_softmax,
csr5hip_row_softmax_grad), on any CSR ``row_ptr``: numpy in ``numpy.longdouble`` (>= 63 bits of mantissa, asserted), vectorised
with ``reduceat`` over the non-empty rows.  Every element is checked.

FORWARD  p[e] = exp(s[e] - M) / Z, M the row's maximum, Z = sum_row exp(s[j] - M).  Datasets (fp64 and fp32, seeded):

* ``uniform``    all scores of a row equal; the value is drawn per row from 0, small integers, +-1e300 (fp64) / +-1e30 (fp32)
                 and the largest finite number.  Every term is exp(0) = 1, Z = L exactly, so the output is exactly dt(1) / dt(L)
                 (reciprocal times 1, or 1 / L: the same correctly rounded value).  Without the subtraction of the maximum the
                 exponentials overflow.
* ``shifted``    integer scores in [-20, 0], and (``shifted_pair``) the same plus an integer per row in +-2**20: s - M is the
                 same exact integer in both, so both outputs are bit-identical, and within the bound.
* ``gaussian``   N(0, 3**2).
* ``wide``       uniform in +-600 (fp64) / +-80 (fp32): terms underflow.
* ``masked``     gaussian with -Inf on about 30 % of the entries, one row entirely -Inf (all NaN), one row with a single
                 survivor (exactly 1); a -Inf score gets exactly +0.
* ``nonfinite``  gaussian with a NaN or a +Inf in a few rows, the first non-empty row always: those rows are all NaN, every other
                 row is within the bound.

Forward bound for a reference p >= the smallest normal number, with d = s - M (exact for the reference; one rounding, delta_1,
in the kernel), u the unit roundoff, c the exponential's error in units of u (``C_EXP``), gamma(n) = n u / (1 - n u):

    |out - p| <= p u [ (|d_e| + c) + sum_j p_j (|d_j| + c) ] (1 + 2**-10)  +  p (gamma(L - 1) + 2 u)

Derivation.  The computed term is t_j = exp(d_j (1 + delta_1)) (1 + c delta_2) = exp(d_j) (1 + eps_j) with |eps_j| <=
u (|d_j| + c) to first order (exp(d delta) = 1 + d delta + ...).  Any summation tree over L non-negative terms gives
Z' = sum t_j (1 + theta_j), |theta_j| <= gamma(L - 1) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), so
Z' / Z = 1 + sum_j p_j eps_j + theta, |theta| <= gamma(L - 1): the relative error of Z is the p-weighted mean of the terms'
errors.  The quotient adds one division, or one reciprocal and one multiplication: at most 2 u.  Together
out / p = (1 + eps_e) / (1 + sum p_j eps_j + theta) (1 + 2u') which is the bound; the factor (1 + 2**-10) covers the second-order
terms (all eps are below 2**-10 for |d| <= 1500 in fp64 and <= 200 in fp32) and the reference's own error (2**-63 relative per
operation, against u >= 2**-53).  A reference below the smallest normal number accepts any output in [0, smallest normal]: how
the device library's exponential rounds in its underflow range is not this feature's business.  There is no other floor.

``C_EXP`` is meant to be measured: scripts/probe_exp_ulp.py runs rows of two entries (d, 0) through the kernel and reports
E = max |out_0 - ref| / (u ref); E bounds the exponential's error from above (it also holds one rounded addition and the two
roundings of the quotient), and C_EXP = ceil(E), with the condition C_EXP <= 8.  THE PROBE HAS NOT BEEN RUN ON A GPU YET
(DESIGN.md section 16), so the constant below is the largest E the probe can report if the device library's exp / expf meet their
documented accuracy of 1 ulp = 2 u: 2 (exponential) + 1 (addition) + 1 (reciprocal) + 1 (multiplication) = 5.  It does not come
from any output of the kernel; replace it by ceil(E) once E is measured.

GRADIENT  out[e] = p[e] (g[e] - D), D = sum_row p[j] g[j].  Datasets:

* ``exact``      p = 2**-q per row, q <= 3; g integers in [-9, 9]: every product is a multiple of 1/8 of magnitude <= 9, every
                 partial sum a multiple of 1/8 of magnitude <= 9 L, every difference and final product likewise exact as long
                 as 72 (L + 1) < 2**24 (fp32) -- asserted for the rows at hand.  Compared exactly.
* ``softmax``    p = the rounded reference softmax of ``gaussian``; g ~ N(0, 1).
* ``nonfinite``  ``softmax`` with NaN in g in a few rows (the first non-empty row always): those rows all NaN, the others bounded.

Gradient bound, for any tree, with or without FMA; S = sum_row |p_j g_j|:

    |out - ref| <= |p_e| [ gamma(L) S + gamma(2) (|g_e - D| + gamma(L) S) ] (1 + 2**-10)

Derivation.  D' = sum p_j g_j (1 + theta_j) with |theta_j| <= gamma(L) (one rounding for the product, at most L - 1 on the way
to the root), so |D' - D| <= gamma(L) S.  The difference and the product round once each: out = p_e (g_e - D') (1 + theta_2),
|theta_2| <= gamma(2), hence |out - p_e (g_e - D)| <= |p_e| [ |D' - D| + gamma(2) |g_e - D'| ] and |g_e - D'| <= |g_e - D| +
gamma(L) S.  (1 + 2**-10) covers the reference's own error.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.exact_reference import unit_roundoff

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs an extended-precision long double"

FORWARD_DATASETS = ("uniform", "shifted", "gaussian", "wide", "masked", "nonfinite")
GRAD_DATASETS = ("exact", "softmax", "nonfinite")
DTYPES = (np.float64, np.float32)
# the exponential's error in units of u: see the module docstring (derived, not yet measured)
C_EXP = {np.float64: 5, np.float32: 5}
WIDE_SPAN = {np.float64: 600.0, np.float32: 80.0}
HUGE = {np.float64: 1e300, np.float32: 1e30}
SLACK = LD(1) + LD(2) ** -10

BOUND, EXACT, ALLNAN, TINY = 0, 1, 2, 3  # how an element is judged


def _key(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def _rows(row_ptr):
    """(lengths, starts of the non-empty rows, their lengths, row index per element)"""
    rp = np.asarray(row_ptr, dtype=np.int64)
    lens = np.diff(rp)
    ne = lens > 0
    return lens, rp[:-1][ne], lens[ne], np.repeat(np.arange(lens.size, dtype=np.int64), lens)


def _per_row(op, a, starts):
    """op.reduceat over the rows (non-empty rows only: consecutive starts delimit exactly the rows)"""
    return op.reduceat(a, starts) if a.size else a[:0]


def _gamma(n, u):
    n = np.asarray(n, dtype=LD)
    return n * u / (LD(1) - n * u)


def make_scores(dataset: str, row_ptr, dtype, seed: int = 0) -> np.ndarray:
    """nnz scores of `dtype` in CSR order"""
    dt = _key(dtype)
    lens, starts, nlens, rows = _rows(row_ptr)
    nnz, m = int(lens.sum()), lens.size
    rng = np.random.default_rng([seed, FORWARD_DATASETS.index(dataset), 64 if dt == np.float64 else 32])
    if dataset == "uniform":
        pool = np.array([0.0, 1.0, -3.0, 7.0, 40.0, HUGE[dt], -HUGE[dt], float(np.finfo(dt).max), -float(np.finfo(dt).max)])
        s = pool[rng.integers(0, pool.size, size=m)][rows]
    elif dataset == "shifted":
        s = rng.integers(-20, 1, size=nnz).astype(np.float64)
    elif dataset == "gaussian":
        s = rng.normal(0.0, 3.0, size=nnz)
    elif dataset == "wide":
        s = rng.uniform(-WIDE_SPAN[dt], WIDE_SPAN[dt], size=nnz)
    elif dataset == "masked":
        s = rng.normal(0.0, 3.0, size=nnz)
        s[rng.random(nnz) < 0.3] = -np.inf
        multi = np.flatnonzero(lens >= 2)
        if multi.size:  # one row entirely -Inf, one row with a single survivor
            rp = np.asarray(row_ptr, dtype=np.int64)
            r0 = int(multi[rng.integers(0, multi.size)])
            s[rp[r0]:rp[r0 + 1]] = -np.inf
            if multi.size > 1:
                r1 = int(multi[(np.flatnonzero(multi == r0)[0] + 1 + rng.integers(0, multi.size - 1)) % multi.size])
                keep = rp[r1] + int(rng.integers(0, lens[r1]))
                s[rp[r1]:rp[r1 + 1]] = -np.inf
                s[keep] = 0.75
    elif dataset == "nonfinite":
        s = rng.normal(0.0, 3.0, size=nnz)
        ne = np.flatnonzero(lens > 0)
        if ne.size:
            rp = np.asarray(row_ptr, dtype=np.int64)
            bad = np.unique(np.concatenate([[ne[0]], rng.choice(ne, size=min(ne.size, 2 + ne.size // 400), replace=False)]))
            for r in bad.tolist():
                s[rp[r] + int(rng.integers(0, lens[r]))] = np.nan if rng.random() < 0.5 else np.inf
    else:
        raise ValueError(dataset)
    return np.ascontiguousarray(s.astype(dt))


def shifted_pair(row_ptr, dtype, seed: int = 0):
    """(s, s + an integer per row in +-2**20): both exact in `dtype`, s - max identical"""
    dt = _key(dtype)
    lens, _, _, rows = _rows(row_ptr)
    s = make_scores("shifted", row_ptr, dt, seed)
    rng = np.random.default_rng([seed, 77])
    shift = rng.integers(-2 ** 20, 2 ** 20 + 1, size=lens.size).astype(np.float64)
    t = (s.astype(np.float64) + shift[rows]).astype(dt)
    assert np.array_equal(t.astype(np.float64) - shift[rows], s.astype(np.float64))
    return s, np.ascontiguousarray(t)


@dataclass
class Reference:
    dtype: type
    expected: np.ndarray   # longdouble (nnz,)
    bound: np.ndarray      # longdouble (nnz,): allowed |out - expected| where kind == BOUND
    kind: np.ndarray       # int8 (nnz,): BOUND, EXACT (value and, for 0, the sign), ALLNAN, TINY (any value in [0, smallest normal])


def softmax_reference(row_ptr, scores, dataset: str = "") -> Reference:
    dt = _key(scores.dtype)
    u = LD(unit_roundoff(dt))
    c = LD(C_EXP[dt])
    tiny = LD(np.finfo(dt).tiny)
    lens, starts, nlens, rows = _rows(row_ptr)
    nnz = int(lens.sum())
    assert scores.shape == (nnz,)
    s = scores.astype(LD)
    expected, bound, kind = np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=np.int8)
    if nnz == 0:
        return Reference(dt, expected, bound, kind)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        M = np.repeat(_per_row(np.fmax, s, starts), nlens)          # (NaN skipped, as the kernel's maximum)
        poisoned = np.repeat(_per_row(np.add, (np.isnan(s) | np.isposinf(s)).astype(np.int64), starts)
                             + (_per_row(np.add, np.isfinite(s).astype(np.int64), starts) == 0), nlens) > 0
        d = np.where(poisoned, LD(0), s - np.where(poisoned, LD(0), M))
        ex = np.exp(d)                                                # exp(-Inf) = 0
        Z = np.repeat(_per_row(np.add, ex, starts), nlens)
        p = ex / Z
        ad = np.where(ex == 0, LD(0), np.abs(np.where(np.isfinite(d), d, LD(0))))  # p_j |d_j| = 0 where p_j = 0
        mean = np.repeat(_per_row(np.add, p * (ad + c), starts), nlens)
        L = np.repeat(nlens, nlens).astype(LD)
        bound[:] = p * u * ((ad + c) + mean) * SLACK + p * (_gamma(L - 1, u) + 2 * u)
    expected[:] = p
    survivors = np.repeat(_per_row(np.add, (~np.isneginf(s)).astype(np.int64), starts), nlens)
    kind[p < tiny] = TINY
    kind[np.isneginf(s) | (survivors == 1)] = EXACT                   # exactly +0, and exactly 1 for a single finite entry
    if dataset == "uniform":
        kind[:] = EXACT
        expected[:] = (dt(1) / L.astype(dt)).astype(LD)
    kind[poisoned] = ALLNAN
    expected[poisoned] = np.nan
    return Reference(dt, expected, bound, kind)


def make_grad(dataset: str, row_ptr, dtype, seed: int = 0):
    """(p, g): nnz values of `dtype` each"""
    dt = _key(dtype)
    lens, starts, nlens, rows = _rows(row_ptr)
    nnz, m = int(lens.sum()), lens.size
    rng = np.random.default_rng([seed, 1000 + GRAD_DATASETS.index(dataset), 64 if dt == np.float64 else 32])
    if dataset == "exact":
        p = np.ldexp(1.0, -rng.integers(0, 4, size=m))[rows]
        g = rng.integers(-9, 10, size=nnz).astype(np.float64)
    else:
        ref = softmax_reference(row_ptr, make_scores("gaussian", row_ptr, dt, seed))
        p = ref.expected.astype(dt)
        g = rng.normal(0.0, 1.0, size=nnz)
        if dataset == "nonfinite":
            ne = np.flatnonzero(lens > 0)
            if ne.size:
                rp = np.asarray(row_ptr, dtype=np.int64)
                bad = np.unique(np.concatenate([[ne[0]], rng.choice(ne, size=min(ne.size, 2 + ne.size // 400), replace=False)]))
                for r in bad.tolist():
                    g[rp[r] + int(rng.integers(0, lens[r]))] = np.nan
        elif dataset != "softmax":
            raise ValueError(dataset)
    return np.ascontiguousarray(p.astype(dt)), np.ascontiguousarray(g.astype(dt))


def grad_reference(row_ptr, p, g, dataset: str = "") -> Reference:
    dt = _key(p.dtype)
    u = LD(unit_roundoff(dt))
    lens, starts, nlens, rows = _rows(row_ptr)
    nnz = int(lens.sum())
    assert p.shape == (nnz,) and g.shape == (nnz,)
    expected, bound, kind = np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=LD), np.zeros(nnz, dtype=np.int8)
    if nnz == 0:
        return Reference(dt, expected, bound, kind)
    pl, gl = p.astype(LD), g.astype(LD)
    with np.errstate(invalid="ignore"):
        pg = pl * gl
        D = np.repeat(_per_row(np.add, pg, starts), nlens)
        S = np.repeat(_per_row(np.add, np.abs(pg), starts), nlens)
        L = np.repeat(nlens, nlens).astype(LD)
        expected[:] = pl * (gl - D)
        gL = _gamma(L, u)
        bound[:] = np.abs(pl) * (gL * S + _gamma(2, u) * (np.abs(gl - D) + gL * S)) * SLACK
    bad = np.isnan(expected)
    kind[bad] = ALLNAN
    if dataset == "exact":
        assert not bad.any()
        # every partial sum is a multiple of 1/8 below 9 L, every output a multiple of 1/64 below 9 (L + 1): exact in `dt`
        assert 72 * (int(nlens.max()) + 1) < 2 ** (np.finfo(dt).nmant + 1), "a row is too long for the exact dataset"
        assert np.array_equal(expected.astype(dt).astype(LD), expected)
        kind[:] = EXACT
    return Reference(dt, expected, bound, kind)


def ratios(out, ref: Reference) -> np.ndarray:
    """|out - expected| / bound of the bounded elements (what a measurement prints before it asserts)"""
    sel = ref.kind == BOUND
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.abs(np.asarray(out).astype(LD)[sel] - ref.expected[sel]) / ref.bound[sel]).astype(np.float64)


def bad_elements(out, ref: Reference) -> np.ndarray:
    out = np.asarray(out)
    assert out.dtype == ref.dtype and out.shape == ref.expected.shape, (out.dtype, out.shape, ref.expected.shape)
    o, e = out.astype(LD), ref.expected
    tiny = LD(np.finfo(ref.dtype).tiny)
    with np.errstate(invalid="ignore"):
        ok_bound = np.abs(o - e) <= ref.bound
        ok_exact = (o == e) & ((e != 0) | ~np.signbit(out))   # an expected 0 is +0
        ok_nan = np.isnan(o)
        ok_tiny = (o >= 0) & (o <= tiny)
    ok = np.select([ref.kind == BOUND, ref.kind == EXACT, ref.kind == ALLNAN], [ok_bound, ok_exact, ok_nan], ok_tiny)
    return np.flatnonzero(~ok)


def check(out, ref: Reference, what="") -> None:
    bad = bad_elements(out, ref)
    if bad.size:
        i = bad[:6]
        raise AssertionError(f"{what}: {bad.size} of {np.asarray(out).size} elements wrong; elements {i.tolist()}: got "
                             f"{np.asarray(out)[i].tolist()}, expected {ref.expected[i].tolist()} (bound "
                             f"{ref.bound[i].tolist()}, kind {ref.kind[i].tolist()})")


def hub_matrix(seed: int = 5):
    """one row of 200 003 entries next to rows of 1, 2, 3, 63, 64, 65 and 0 entries (and one of each class boundary)"""
    from benchmark_spmv_using_csr5_amd import matrices as M
    lengths = [1, 2, 3, 0, 63, 64, 65, 200003, 0, 4, 5, 16, 17, 512, 513, 2048, 2049, 1, 0, 3000]
    return M.csr_from_row_lengths(np.asarray(lengths), 4096, np.random.default_rng(seed), name="hub-row")
