"""Patterns and EXACT expectations for the attention kernels at the places where they decide things (numpy only, no GPU): the
edges of the line classes, hub lines beyond workgroup 0, and line counts at which the head groups of the packed calls hold
three heads or all of them.  Used by tests/test_gpu_attention_edges.py, tests/test_attention_edges_host.py and the host-emulation
scripts (scripts/host_emulation/emulation.py for run_*.py).

THE CLASSES (csr5_attention_dev.h): a line of at most AT_G = 16 entries is taken by 16 lanes, one of 17 .. AT_WAVE_ROW = 512 by a
wavefront, a longer one ("hub") by the workgroup after a barrier; up to AT_STAGE = 2 048 entries a hub is staged once, beyond
that it is recomputed chunk by chunk of 2 048.  A workgroup owns AT_BLOCK = 256 consecutive lines, a wavefront 64 of them.

THE EXACT EXPECTATIONS rest on operands for which every intermediate of the definition (csr5hip.h, csr5_attention.hip,
csr5_attention_bwd.hip) is exact in fp32, whatever the summation order:

* forward: every unmasked score is exactly +0 (a chain of fused multiply-adds of +-0 products onto +0), so M = +0, every weight
  is exp(0) = 1 and Z is the count |U| of the row's unmasked entries (with multiplicity); a masked score is -Inf and its weight
  exp(-Inf) = +0.  V holds integers, so every partial sum of w V is an integer, exact while the sum of |V| over U stays below
  2**24.  What is left is the definition's ONE correctly rounded reciprocal and ONE product:
  O[i, c] = fl(fl(1 / |U|) * sum_U V[j_e, c]); NaN where the row has entries and all are masked (M = -Inf, -Inf - -Inf); +0 for
  a row without entries.  A sum that cancels gives +0 (round to nearest; every chain starts from +0 and w >= +0).
* backward on a pattern whose rows all hold exactly 16 entries, with Q = 0 or K = 0 and integer operands: s = +0, w = 1,
  r = 1/16, p = 1/16; dp is an integer; round(p dp) = dp / 16 exactly, so 16 D is an integer; 256 ds = 16 dp - 16 D is an
  integer; dQ and dK are integers over 256, dV integers over 16.  Exact in every order while, for every output element and
  every D, the sum of the absolute terms in those units stays below 2**24 (`ExactBackward.worst`)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from benchmark_spmv_using_csr5_amd import matrices as M

AT_BLOCK, AT_G, AT_WAVE_ROW, AT_STAGE = 256, 16, 512, 2048
AT_GRID_TARGET = 1024
CYCLE = (0, 1, 15, 16, 17, 63, 64, 65, 511, 512)
# row -> length: why each is there is the table in tests/test_gpu_attention_edges.py
OVERRIDES = {3: 513, 60: 2048, 61: 2049, 130: 4096, 256: 4097, 511: 513, 700: 2049, 768: 600}
EDGE_M, EDGE_N = 3 * AT_BLOCK + 1, 4608
PADDED_COLUMN = 768  # dealt(): the column that takes the padding entries
EXACT_LIMIT = 2 ** 24
HUGE = {np.float64: -1e308, np.float32: -3e38}  # times 2 it overflows to -Inf


def _key(dtype):
    return np.float64 if np.dtype(dtype) == np.float64 else np.float32


def heads_per_group(lines: int, heads: int) -> int:
    """att_heads_per_group of csr5_attention_dev.h, transcribed: the heads one workgroup of a packed launch takes"""
    blocks = (lines + AT_BLOCK - 1) // AT_BLOCK if lines > 0 else 1
    groups = (AT_GRID_TARGET + blocks - 1) // blocks
    groups = max(min(groups, (heads + 1) // 2), 1)
    return (heads + groups - 1) // groups


def edge_lengths() -> np.ndarray:
    lengths = np.array([CYCLE[i % len(CYCLE)] for i in range(EDGE_M)], dtype=np.int64)
    for row, length in OVERRIDES.items():
        lengths[row] = length
    return lengths


def class_edges():
    """769 x 4 608: a line on either side of every class edge in every wavefront, hubs in workgroups 0, 1 and 2 and alone in 3;
    columns unsorted, duplicates allowed"""
    return M.csr_from_row_lengths(edge_lengths(), EDGE_N, np.random.default_rng(77), name="class-edges")


def dealt():
    """7 012 x 769 with exactly 16 entries in every row, whose COLUMN lengths are class_edges()' row lengths (column 768 padded
    to make the total a multiple of 16): entry t, in column order, goes to row perm[t] // 16"""
    lengths = edge_lengths()
    lengths[PADDED_COLUMN] += -int(lengths.sum()) % AT_G
    total = int(lengths.sum())
    cols = np.repeat(np.arange(lengths.size, dtype=np.int64), lengths)
    rows = np.random.default_rng(78).permutation(total) // AT_G
    order = np.argsort(rows, kind="stable")
    row_ptr = np.arange(0, total + 1, AT_G, dtype=np.int32)
    return M.CsrMatrix(total // AT_G, lengths.size, row_ptr, cols[order].astype(np.int32), np.zeros(total), "dealt")


def many_lines(m: int):
    """m x m with rows of 0 .. 3 entries, one row of 40 entries (the wavefront class) in the middle at an index 256 q + 63 and one
    of 513 entries (a hub) as the very last row; for m = 256 q' + 1 that hub is the only line of the last workgroup"""
    rng = np.random.default_rng([79, m])
    lengths = rng.integers(0, 4, size=m).astype(np.int64)
    lengths[middle_row(m)] = 40
    lengths[m - 1] = AT_WAVE_ROW + 1
    return M.csr_from_row_lengths(lengths, m, rng, name=f"many-lines-{m}")


def middle_row(m: int) -> int:
    return AT_BLOCK * ((m // 2) // AT_BLOCK) + 63


def rows_of(mat) -> np.ndarray:
    return np.repeat(np.arange(mat.m, dtype=np.int64), np.diff(mat.row_ptr))


# ---- exact forward -------------------------------------------------------------------------------------------------------------
VARIANTS = ("k0", "q0", "masked")


def forward_operands(mat, variant: str, k: int, d: int, dtype, seed: int, heads: int = 0):
    """(Q, K, V, unmasked): V integers in [-1000, 1000]; every unmasked score exactly +0; unmasked[e] (or [h][e] with heads) tells
    whether entry e, in CSR order, carries weight 1 (otherwise +0).  With heads the operands are packed (rows, heads, width) and
    every head has values and a mask of its own.
      k0      k = 0: no score chain at all
      q0      Q = +0, K uniform in [-1, 1)
      masked  K[:, 0] in {0, 2} (about 60 % zeros), Q[:, 0] = -huge, the rest of Q +0 and of K uniform: -huge * 2 = -Inf"""
    dt = _key(dtype)
    H = max(heads, 1)
    rng = np.random.default_rng([seed, VARIANTS.index(variant), k, d, H, 64 if dt == np.float64 else 32])
    if variant == "k0":
        assert k == 0
    Q = np.zeros((mat.m, H, k), dtype=dt)
    K = rng.uniform(-1, 1, size=(mat.n, H, k)).astype(dt)
    V = rng.integers(-1000, 1001, size=(mat.n, H, d)).astype(dt)
    cols = mat.col[:mat.nnz].astype(np.int64)
    unmasked = np.ones((H, mat.nnz), dtype=bool)
    if variant == "masked":
        K[:, :, 0] = np.where(rng.random((mat.n, H)) < 0.6, 0, 2)
        Q[:, :, 0] = HUGE[dt]
        unmasked = np.ascontiguousarray((K[:, :, 0] == 0)[cols].T)
    if heads:
        return Q, K, V, unmasked
    return Q[:, 0], K[:, 0], V[:, 0], unmasked[0]


def exact_forward(mat, V, unmasked, dtype):
    """(O, largest sum of |V| over a row's unmasked entries): the module docstring's expectation, in int64 with one reciprocal
    and one product rounded in `dtype`; the second value must stay below EXACT_LIMIT for O to be order-independent in fp32"""
    dt = _key(dtype)
    Vi = np.asarray(V).astype(np.int64)
    assert np.array_equal(Vi.astype(dt), V), "V must hold integers"
    rows, cols = rows_of(mat)[unmasked], mat.col[:mat.nnz].astype(np.int64)[unmasked]
    sums, mags = np.zeros((mat.m, Vi.shape[1]), dtype=np.int64), np.zeros((mat.m, Vi.shape[1]), dtype=np.int64)
    np.add.at(sums, rows, Vi[cols])
    np.add.at(mags, rows, np.abs(Vi[cols]))
    count = np.bincount(rows, minlength=mat.m)
    O = np.zeros(sums.shape, dtype=dt)
    some = count > 0
    O[some] = (dt(1) / count[some].astype(dt))[:, None] * sums[some].astype(dt)
    O[(np.diff(mat.row_ptr) > 0) & ~some] = np.nan
    return O, int(mags.max()) if mags.size else 0


def mask_conditions(mat, unmasked):
    """(every row of 17 or more entries keeps a masked and an unmasked entry, share of all-masked rows among the non-empty ones)"""
    lens = np.diff(mat.row_ptr)
    kept = np.bincount(rows_of(mat)[unmasked], minlength=mat.m)
    longer = lens > AT_G
    mixed = bool(((kept[longer] > 0) & (kept[longer] < lens[longer])).all())
    return mixed, float(((lens > 0) & (kept == 0)).sum()) / max(int((lens > 0).sum()), 1)


def same_bits(got, want) -> bool:
    """bit for bit, sign of zero included; where NaN is expected any NaN will do"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    word = np.uint64 if got.dtype == np.float64 else np.uint32
    return bool(np.isnan(got[nan]).all()) and np.array_equal(got.view(word)[~nan], want.view(word)[~nan])


# ---- exact backward ------------------------------------------------------------------------------------------------------------
def backward_operands(mat, zero: str, k: int, d: int, dtype, seed: int, heads: int = 0):
    """(Q, K, V, dO) of integers in [-2, 2] with Q (zero = "Q": dQ is the non-trivial output) or K (zero = "K": dK) all +0;
    packed (rows, heads, width) with heads"""
    dt = _key(dtype)
    H = max(heads, 1)
    rng = np.random.default_rng([seed, "QK".index(zero), k, d, H, 64 if dt == np.float64 else 32])
    Q, K, V, dO = (rng.integers(-2, 3, size=(r, H, w)).astype(dt) for r, w in ((mat.m, k), (mat.n, k), (mat.n, d), (mat.m, d)))
    (Q if zero == "Q" else K)[:] = 0
    if heads:
        return Q, K, V, dO
    return Q[:, 0], K[:, 0], V[:, 0], dO[:, 0]


@dataclass
class ExactBackward:
    dQ: np.ndarray
    dK: np.ndarray
    dV: np.ndarray
    worst: int  # the largest sum of absolute terms of any output element or D, in its unit (1/256, 1/256, 1/16, 1/16)


def exact_backward(mat, Q, K, V, dO, dtype) -> ExactBackward:
    """the module docstring's expectation on a pattern with 16 entries in every row and all scores +0, in int64"""
    dt = _key(dtype)
    assert (np.diff(mat.row_ptr) == AT_G).all(), "every row must hold exactly 16 entries"
    Qi, Ki, Vi, dOi = (np.asarray(t).astype(np.int64) for t in (Q, K, V, dO))
    assert all(np.array_equal(i.astype(dt), t) for i, t in zip((Qi, Ki, Vi, dOi), (Q, K, V, dO))), "integer operands"
    assert not Qi.any() or not Ki.any(), "Q or K must be zero: every score is +0"
    rows, cols = rows_of(mat), mat.col[:mat.nnz].astype(np.int64)
    dp = (dOi[rows] * Vi[cols]).sum(axis=1)                                  # integers
    D16 = np.bincount(rows, dp, minlength=mat.m).astype(np.int64)            # 16 D
    ds256 = AT_G * dp - D16[rows]                                            # 256 ds

    def scatter(idx, n, terms):
        out, mag = np.zeros((n, terms.shape[1]), dtype=np.int64), np.zeros((n, terms.shape[1]), dtype=np.int64)
        np.add.at(out, idx, terms)
        np.add.at(mag, idx, np.abs(terms))
        return out, int(mag.max()) if mag.size else 0
    dQ, wq = scatter(rows, mat.m, ds256[:, None] * Ki[cols])
    dK, wk = scatter(cols, mat.n, ds256[:, None] * Qi[rows])
    dV, wv = scatter(cols, mat.n, dOi[rows])
    wd = int(np.bincount(rows, np.abs(dp), minlength=mat.m).max())
    worst = max(wq, wk, wv, wd, int(np.abs(ds256).max()))
    return ExactBackward(dQ.astype(dt) / dt(256), dK.astype(dt) / dt(256), dV.astype(dt) / dt(16), worst)
