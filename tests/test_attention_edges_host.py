"""tests/attention_edges.py on the host (no GPU): the patterns have the line lengths and workgroup positions that
tests/test_gpu_attention_edges.py relies on, the transcription of the head-group rule gives the splits that test wants and agrees
with the header it transcribes, the 2**24 conditions hold on the GPU tests' own operands, and the exact-expectation calculators
agree with a slow per-row computation in Python ``fractions`` on a 30-row cut."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from benchmark_spmv_using_csr5_amd import matrices as M
from tests import attention_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.float64, np.float32)


def test_the_constants_are_the_headers():
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_attention_dev.h")) as f:
        text = f.read()
    for name, value in (("AT_BLOCK", E.AT_BLOCK), ("AT_G", E.AT_G), ("AT_WAVE_ROW", E.AT_WAVE_ROW)):
        assert re.search(rf"constexpr int {name} = {value};", text), name
    assert "AT_STAGE = AT_WAVES * AT_WAVE_ROW;" in text and "AT_WAVES = AT_BLOCK / OMEGA;" in text
    assert E.AT_STAGE == (E.AT_BLOCK // 64) * E.AT_WAVE_ROW
    assert re.search(rf"constexpr long long AT_GRID_TARGET = {E.AT_GRID_TARGET};", text)


def test_class_edges_has_a_line_on_every_edge_and_hubs_in_every_workgroup():
    mat = E.class_edges()
    lens = np.diff(mat.row_ptr)
    assert (mat.m, mat.n, mat.nnz) == (769, 4608, 112188) and mat.m == 3 * E.AT_BLOCK + 1
    assert {0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2048, 2049, 4096, 4097} <= set(lens.tolist())
    for row, length in E.OVERRIDES.items():
        assert lens[row] == length
    plain = np.setdiff1d(np.arange(mat.m), list(E.OVERRIDES))
    assert np.array_equal(lens[plain], np.array(E.CYCLE)[plain % 10])
    # where the hubs lie: workgroup, wavefront, lane
    hubs = {int(r): (int(r) // 256, int(r) % 256 // 64, int(r) % 64) for r in np.flatnonzero(lens > E.AT_WAVE_ROW)}
    assert hubs == {3: (0, 0, 3), 60: (0, 0, 60), 61: (0, 0, 61), 130: (0, 2, 2), 256: (1, 0, 0), 511: (1, 3, 63), 700: (2, 2, 60),
                    768: (3, 0, 0)}
    assert lens[60] == E.AT_STAGE and lens[61] == E.AT_STAGE + 1 and lens[130] == 2 * E.AT_STAGE and lens[256] == 2 * E.AT_STAGE + 1
    for wg in range(3):  # every full workgroup: hubs beside wavefront-class rows and short rows in every wavefront
        for wave in range(4):
            part = lens[wg * 256 + wave * 64:wg * 256 + wave * 64 + 64]
            assert ((part > E.AT_G) & (part <= E.AT_WAVE_ROW)).any() and (part <= E.AT_G).any()
            assert {16, 17, 63, 64, 65, 511, 512} <= set(part.tolist())
    assert mat.m - 1 == 768 and (mat.m - 1) % E.AT_BLOCK == 0  # the last workgroup holds that one row
    cols = np.bincount(mat.col[:mat.nnz], minlength=mat.n)
    assert cols.max() == 42  # the transpose's rows are short: its columns are what the column kernel's classes see
    row0 = mat.col[mat.row_ptr[256]:mat.row_ptr[257]]
    assert (np.diff(row0) < 0).any() and np.unique(row0).size < row0.size  # unsorted, with duplicates


def test_dealt_has_sixteen_entries_in_every_row_and_the_edge_lengths_in_its_columns():
    mat = E.dealt()
    assert (mat.m, mat.n, mat.nnz) == (7012, 769, 112192)
    assert (np.diff(mat.row_ptr) == 16).all()
    cols = np.bincount(mat.col[:mat.nnz], minlength=mat.n)
    want = E.edge_lengths()
    want[E.PADDED_COLUMN] += 4
    assert np.array_equal(cols, want) and cols[E.PADDED_COLUMN] == 604 and mat.nnz % 16 == 0
    rows = E.rows_of(mat)
    for c in (61, 256):  # a long column's entries are spread over the rows, not bunched
        assert np.unique(rows[mat.col[:mat.nnz] == c]).size > 0.6 * cols[c]


@pytest.mark.parametrize("m", (90113, 262145))
def test_many_lines_ends_in_a_workgroup_of_one_hub(m):
    mat = E.many_lines(m)
    lens = np.diff(mat.row_ptr)
    mid = E.middle_row(m)
    assert mat.m == mat.n == m and (m - 1) % E.AT_BLOCK == 0
    assert lens[m - 1] == 513 and lens[mid] == 40 and mid % E.AT_BLOCK == 63 and m // 4 < mid < 3 * m // 4
    rest = np.delete(lens, [mid, m - 1])
    assert rest.max() == 3 and rest.min() == 0


def test_the_head_group_rule_gives_the_intended_splits():
    assert E.heads_per_group(90113, 8) == 3          # 3 + 3 + 2
    assert [min(3, 8 - 3 * g) for g in range((8 + 2) // 3)] == [3, 3, 2]
    assert E.heads_per_group(262145, 8) == 8 and E.heads_per_group(262145, 5) == 5 and E.heads_per_group(262145, 3) == 3
    # what the rest of the GPU suite gets: one or two heads, up to the line counts of the comments in csr5_attention_dev.h
    for lines in (0, 1, 40, 769, 7012, 30000):
        for heads in (1, 2, 3, 5, 8):
            assert E.heads_per_group(lines, heads) == min(heads, 2), (lines, heads)
    assert E.heads_per_group(341 * 256, 8) == 2 and E.heads_per_group(341 * 256 + 1, 8) == 3   # 342 workgroups: three heads
    assert E.heads_per_group(1023 * 256, 8) == 4 and E.heads_per_group(1023 * 256 + 1, 8) == 8  # 1 024 workgroups: all heads


def test_the_transcription_is_the_headers_function(tmp_path):
    """the header's rule compiled for the host against the transcription, on a grid of (lines, heads)"""
    import subprocess
    src = tmp_path / "rule.cpp"
    src.write_text(
        "#include <cstdio>\n"
        "constexpr int AT_BLOCK = 256;\n"
        + _rule_text() +
        "int main() { const long long L[] = {0, 1, 255, 256, 257, 769, 7012, 87296, 87297, 90113, 131072, 131073, 262144, 262145, 1000000};\n"
        "  for (long long l : L) for (int h = 1; h <= 9; h++) std::printf(\"%lld %d %d\\n\", l, h, att_heads_per_group(l, h)); }\n")
    exe = tmp_path / "rule"
    r = subprocess.run(["g++", "-std=c++14", "-O0", str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    rows = np.array(out, dtype=np.int64).reshape(-1, 3)
    assert rows.shape[0] == 15 * 9
    for lines, heads, got in rows.tolist():
        assert E.heads_per_group(lines, heads) == got, (lines, heads)


def _rule_text():
    with open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_attention_dev.h")) as f:
        text = f.read()
    start = text.index("constexpr long long AT_GRID_TARGET")
    end = text.index("}\n", text.index("inline int att_heads_per_group", start)) + 2
    return text[start:end]


# ---- the exact expectations against Python fractions on a 30-row cut -----------------------------------------------------------
def _cut(mat, rows):
    lens = np.diff(mat.row_ptr)[rows]
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum(lens)
    col = np.concatenate([mat.col[mat.row_ptr[r]:mat.row_ptr[r + 1]] for r in rows]).astype(np.int32)
    return M.CsrMatrix(len(rows), mat.n, rp, col, np.ones(col.size), mat.name + "-cut")


def _round(frac, dtype):
    """a Fraction rounded to `dtype` once (through float64: exact here, every value fits 53 bits)"""
    value = frac.numerator / frac.denominator
    assert Fraction(value) == frac or dtype == np.float64
    return dtype(value)


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_exact_forward_agrees_with_fractions_on_a_cut(dtype):
    mat = E.class_edges()
    rows = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 60, 61, 130, 256, 511, 700, 768] + list(range(10, 23))
    assert len(rows) == 30
    cut = _cut(mat, rows)
    for variant, k, d, seed in (("k0", 0, 17, 1), ("q0", 8, 5, 1), ("masked", 5, 65, 2)):
        Q, K, V, unmasked = E.forward_operands(cut, variant, k, d, dtype, seed)
        assert not Q[:, 1:].any() and (variant != "masked" or (Q[:, 0] == E.HUGE[dtype]).all())
        got, worst = E.exact_forward(cut, V, unmasked, dtype)
        assert worst < E.EXACT_LIMIT
        seen_nan = False
        for i in range(cut.m):
            a, b = int(cut.row_ptr[i]), int(cut.row_ptr[i + 1])
            kept = [int(cut.col[e]) for e in range(a, b) if unmasked[e]]
            if variant == "masked":  # the mask is the score's: -huge * 2 = -Inf, -huge * 0 = -0
                with np.errstate(over="ignore"):
                    assert kept == [int(j) for j in cut.col[a:b] if np.isfinite(Q[i, 0] * K[j, 0])]
            for c in range(d):
                if b == a:
                    assert got[i, c] == 0 and not np.signbit(got[i, c])
                elif not kept:
                    assert np.isnan(got[i, c])
                    seen_nan = True
                else:
                    r = dtype(1) / dtype(len(kept))  # ONE correctly rounded reciprocal
                    total = sum(int(V[j, c]) for j in kept)
                    want = dtype(float(Fraction(float(r)) * total))  # ONE product, rounded once (the product fits a double)
                    assert Fraction(float(r)) * total == Fraction(float(Fraction(float(r)) * total)) or dtype == np.float64
                    assert got[i, c] == want and np.signbit(got[i, c]) == np.signbit(want), (variant, i, c)
        assert seen_nan == (variant == "masked")


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_exact_backward_agrees_with_fractions_on_a_cut(dtype):
    mat = E.dealt()
    cut = _cut(mat, list(range(30)))
    for zero in ("Q", "K"):
        Q, K, V, dO = E.backward_operands(cut, zero, 3, 4, dtype, seed=3)
        got = E.exact_backward(cut, Q, K, V, dO, dtype)
        assert got.worst < E.EXACT_LIMIT
        p = Fraction(1, 16)
        dQ = [[Fraction(0)] * 3 for _ in range(cut.m)]
        dK = [[Fraction(0)] * 3 for _ in range(cut.n)]
        dV = [[Fraction(0)] * 4 for _ in range(cut.n)]
        for i in range(cut.m):
            js = [int(j) for j in cut.col[cut.row_ptr[i]:cut.row_ptr[i + 1]]]
            dp = [sum(Fraction(int(dO[i, c])) * int(V[j, c]) for c in range(4)) for j in js]
            D = sum(p * x for x in dp)
            for j, x in zip(js, dp):
                ds = p * (x - D)
                for c in range(3):
                    dQ[i][c] += ds * int(K[j, c])
                    dK[j][c] += ds * int(Q[i, c])
                for c in range(4):
                    dV[j][c] += p * int(dO[i, c])
        for g, w in ((got.dQ, dQ), (got.dK, dK), (got.dV, dV)):
            want = np.array([[_round(x, dtype) for x in row] for row in w], dtype=dtype)
            assert np.array_equal(g, want) and not np.signbit(g[g == 0]).any()
        assert (got.dQ if zero == "Q" else got.dK).any() and not (got.dK if zero == "Q" else got.dQ).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp64", "fp32"))
def test_the_exactness_conditions_hold_on_the_gpu_tests_operands(dtype):
    """what tests/test_gpu_attention_edges.py asserts before it compares bits, evaluated here as well"""
    mat = E.class_edges()
    for variant, k, d, seed in (("k0", 0, 17, 1), ("q0", 8, 5, 1), ("masked", 5, 65, 2), ("masked", 8, 16, 2)):
        for heads in (0, 3):
            Q, K, V, unmasked = E.forward_operands(mat, variant, k, d, dtype, seed, heads=heads)
            for h in range(max(heads, 1)):
                v, um = (V[:, h], unmasked[h]) if heads else (V, unmasked)
                assert np.abs(v).max() <= 1000 and E.exact_forward(mat, v, um, dtype)[1] < E.EXACT_LIMIT
                if variant == "masked":
                    mixed, all_masked = E.mask_conditions(mat, um)
                    assert mixed and 0 < all_masked < 0.1
    mat = E.dealt()
    worst = 0
    for zero in ("Q", "K"):
        for k, d in ((8, 5), (3, 17)):
            worst = max(worst, E.exact_backward(mat, *E.backward_operands(mat, zero, k, d, dtype, seed=3), dtype).worst)
            ops = E.backward_operands(mat, zero, k, d, dtype, seed=4, heads=3)
            for h in range(3):
                worst = max(worst, E.exact_backward(mat, *(t[:, h] for t in ops), dtype).worst)
    assert 1e5 < worst < E.EXACT_LIMIT / 8  # about 5e5: far from the limit


def test_same_bits_tells_the_sign_of_zero_and_takes_any_nan():
    for dtype in DTYPES:
        a = np.array([0.0, 1.5, np.nan], dtype=dtype)
        assert E.same_bits(a, a.copy())
        assert not E.same_bits(np.array([-0.0, 1.5, np.nan], dtype=dtype), a)
        assert not E.same_bits(np.array([0.0, 1.5, 2.0], dtype=dtype), a)
        assert not E.same_bits(np.array([0.0, np.nan, np.nan], dtype=dtype), a)
        assert E.same_bits(np.array([0.0, 1.5, -np.nan], dtype=dtype), a)
