"""tests/slab_child_reference.py -- the host model the GPU structure tests (test_gpu_slab_child.py) hold the hot slab child against -- pinned down
on cases small enough to check by hand: a table of 4 to 8 slots and min_count 2 put the table-full regime on a dozen columns, and a child
sigma of 1 makes tiles of 64 elements.  Every expected number below was worked out from the rule (the model's docstring), by hand.  The second
half damages copies of a correct model, one array at a time, and wants compare() to name the array and the first differing index.

All columns of the selection cases lie in slab 0 of the map (bits 3, shift 0): 0, 9, 18, 27, 36, 45, 54, 63, 65, 72 (the xor of their 3-bit
groups is 0); their local ids are col >> 3 and their hashes (c * 2654435761 mod 2^32) >> 21 are 0, 1151, 255, 1406, 510, 1662, 765, 1917, 352, 1020."""
import numpy as np
import pytest

from tests import slab_child_reference as R

SLAB0 = [0, 9, 18, 27, 36, 45, 54, 63, 65, 72]
HASHES = [0, 1151, 255, 1406, 510, 1662, 765, 1917, 352, 1020]
# uses: two columns 5 times, two 4 times, four 3 times, two twice
USES = {9: 5, 27: 5, 18: 4, 45: 4, 0: 3, 36: 3, 54: 3, 63: 3, 65: 2, 72: 2}


def _select(capacity, min_count=2):
    counts = [USES[c] for c in SLAB0]
    chosen, thr, second, admitted, buckets = R.select_table(SLAB0, counts, 0, 3, capacity, min_count)
    return list(chosen), thr, sorted(second), sorted(admitted)


def test_hash_and_map_of_the_hand_cases():
    assert list(R.hot_hash(SLAB0)) == HASHES
    assert [(c * 2654435761 % 2 ** 32) >> 21 for c in SLAB0] == HASHES
    assert set(R.slab_of(SLAB0, 0, 3)) == {0}
    assert list(R.slab_local(SLAB0, 0, 3)) == [c >> 3 for c in SLAB0]


def test_threshold_above_min_count_and_a_second_class_partly_admitted():
    """6 slots, 5 in use at most: 10 columns were used twice, 8 three times, 4 four times -> thr 4, one slot is left for the class of 3 uses
    (0, 36, 54, 63: hash order 0 < 510 < 765 < 1917): the leading buckets 0 .. 509 hold column 0 alone and fit, bucket 510 would make two"""
    chosen, thr, second, admitted = _select(6)
    assert thr == 4 and second == [0, 36, 54, 63] and admitted == [0]
    assert chosen == [0, 9, 18, 27, 45]  # slots 1 .. 5 in local-id order
    chosen, thr, second, admitted = _select(8)  # 7 in use at most: three slots are left, 0, 36 and 54 fit, 63 does not
    assert thr == 4 and admitted == [0, 36, 54] and chosen == [0, 9, 18, 27, 36, 45, 54]
    chosen, thr, second, admitted = _select(7)
    assert thr == 4 and admitted == [0, 36] and chosen == [0, 9, 18, 27, 36, 45]


def test_second_class_not_admitted_and_absent():
    chosen, thr, second, admitted = _select(5)  # 4 in use at most: the first class fills the table
    assert thr == 4 and second == [0, 36, 54, 63] and admitted == [] and chosen == [9, 18, 27, 45]
    chosen, thr, second, admitted = _select(4)  # 3 at most: thr 5, the class of 4 uses (18: 255, 45: 1662) gets one slot
    assert thr == 5 and second == [18, 45] and admitted == [18] and chosen == [9, 18, 27]
    chosen, thr, second, admitted = _select(16)  # everything fits at min_count: no second class (count 1 < min_count)
    assert thr == 2 and second == [] and chosen == sorted(SLAB0)
    chosen, thr, second, admitted = _select(9)  # 8 at most: thr 3, the class of 2 uses finds no room
    assert thr == 3 and second == [65, 72] and admitted == [] and len(chosen) == 8


def test_a_second_class_is_never_wholly_admitted():
    """thr is the SMALLEST fitting count: if the whole class of thr - 1 uses fitted, thr - 1 would fit.  So 'wholly admitted' cannot occur, and
    the room is always smaller than the class: checked on random slabs"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        ncols, capacity = int(rng.integers(1, 40)), int(rng.integers(4, 9))
        cols = R.slab_column(0, np.sort(rng.choice(500, size=ncols, replace=False)), 0, 3)
        counts = rng.integers(1, 7, size=ncols)
        chosen, thr, second, admitted, _ = R.select_table(cols, counts, 0, 3, capacity, 2)
        assert len(chosen) <= capacity - 1
        assert len(second) == 0 or len(admitted) < len(second)
        assert thr == 2 or np.count_nonzero(counts >= thr - 1) > capacity - 1
        assert sorted(R.slab_local(chosen, 0, 3)) == list(R.slab_local(chosen, 0, 3))


def test_counts_are_capped_at_the_last_bucket():
    """5 000 and 2 047 uses are one class (bucket 2 047): with one slot for the two of them thr is 2 048 -- no first class -- and the second class
    takes its one slot in hash order (9: 1151, 18: 255)"""
    chosen, thr, second, admitted, _ = R.select_table([9, 18], [5000, 2047], 0, 3, 2, 2)
    assert thr == 2048 and sorted(second) == [9, 18] and list(chosen) == [18]


@pytest.mark.parametrize("bits,shift", [(3, 4), (4, 0), (3, 2), (5, 4)])
def test_slab_column_inverts_slab_local(bits, shift):
    c = np.arange(70000)
    k, local = R.slab_of(c, shift, bits), R.slab_local(c, shift, bits)
    assert k.max() == (1 << bits) - 1 and local.max() < R.slab_local_count(c.size, shift, bits)
    assert np.array_equal(R.slab_column(k, local, shift, bits), c)
    for s in range(1 << bits):  # dense and in column order inside a slab
        mine = local[k == s]
        assert np.all(np.diff(mine) > 0)


def _two_slab_matrix():
    """21 rows.  Rows 0 .. 19: columns 0 9 (slab 0) and 1 8 19 26 37 (slab 1); row 20: column 19.  141 non-zeros, S = 8, bits 3, shift 0, tiles
    of 64: the child is 40 elements of slab 0 (20 rows of 2), then 101 of slab 1 (20 rows of 5, one of 1); tile 0 = elements 0 .. 63 belongs to
    slab 0 and ends with rows 0 .. 3 and four elements of row 4 of slab 1; tile 1 belongs to slab 1; elements 128 .. 140 are the CSR tail."""
    rows = [[0, 1, 8, 9, 19, 26, 37]] * 20 + [[19]]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return 21, 38, row_ptr, np.concatenate(rows)


@pytest.fixture(scope="module")
def two_slabs():
    m, n, row_ptr, col = _two_slab_matrix()
    return R.build_model(m, n, row_ptr, col, S=8, shift=0, value_size=8, capacity=6, min_count=2, sigma=1)


def test_child_and_empty_slabs(two_slabs):
    mo = two_slabs
    assert (mo["T"], mo["p"], mo["segments"]) == (64, 3, 41)
    assert list(mo["slab_off"]) == [0, 40] + [141] * 7
    assert list(mo["col"][:4]) == [0, 9, 0, 9] and list(mo["col"][40:46]) == [1, 8, 19, 26, 37, 1] and mo["col"][140] == 19
    assert list(mo["row_ptr"][:3]) == [0, 2, 4] and list(mo["row_ptr"][20:23]) == [40, 45, 50] and list(mo["row_ptr"][-2:]) == [140, 141]
    assert list(mo["tile0"]) == [0, 1] + [2] * 7  # slabs 2 .. 7 own no column: no tile, equal offsets
    assert list(mo["hot_count"]) == [3, 6] + [1] * 6
    assert list(mo["hot_cols"][0]) == [0, 0, 9, 0, 0, 0] and list(mo["hot_cols"][1]) == [0, 1, 8, 19, 26, 37] and not mo["hot_cols"][2:].any()
    assert mo["covered"] == 141 and mo["cover_pct"] == 100
    assert np.all(mo["range_begin"][2:] == 2)  # 257 equal words per slab without a column


def test_a_hot_column_behind_its_tiles_slab_end_is_cold_and_ties_go_by_local_id(two_slabs):
    mo = two_slabs
    # elements 40 .. 63: slab 1's, inside slab 0's tile -> cold although every column of theirs has a slot in slab 1
    assert mo["foreign_hot"].sum() == 24 and mo["foreign_hot"][40:64].all() and mo["hot"][:40].all() and mo["hot"][64:].all()
    # cold region of slab 1: 19 (21 uses) first, then 1 8 26 37 (20 uses each) by local id; slab 0 has none
    assert list(mo["cold_base"]) == [0, 0] + [5] * 7 and list(mo["cold_cols"]) == [19, 1, 8, 26, 37]
    code = mo["code"]
    assert code.size == 128
    assert [hex(c) for c in code[:3]] == ["0xc00001", "0x800002", "0xc00001"]  # slot 1 | row start, slot 2
    assert [hex(c) for c in code[40:46]] == ["0x400001", "0x2", "0x0", "0x3", "0x4", "0x400001"]  # cold ranks of 1 8 19 26 37; row starts
    assert [hex(c) for c in code[64:67]] == ["0x800005", "0xc00001", "0x800002"]  # tile 1 runs with slab 1's table: 37, then row 5: 1 8
    assert list(mo["col_lo"][40:42]) == [1, 2] and list(mo["col_hi"][40:42]) == [0x40, 0] and mo["col_hi"][0] == 0xC0
    assert np.array_equal(R.decode(mo), mo["col"][:128])


def test_costs_cuts_and_heads(two_slabs):
    mo = two_slabs
    assert R.cost_constants() == (195, -262, 16)  # (the numbers below are worked out with these)
    # tile 0: 24 cold lanes, 20 + 5 row starts; tile 1: none cold, rows 5 .. 17 of slab 1 start in it
    assert list(mo["tile_cold"]) == [24, 0] and list(mo["tile_starts"]) == [25, 13]
    assert list(mo["range_cost"]) == [0, 195 * 64 - 262 * 24 + 16 * 25, 6592 + 195 * 64 + 16 * 13]
    # one tile per slab: range 0 takes it, the other 255 are empty
    assert list(mo["range_begin"][0][:3]) == [0, 1, 1] and mo["range_begin"][0][256] == 1
    assert list(mo["range_begin"][1][:3]) == [1, 2, 2]
    head = mo["range_head"]
    assert head.size == 8 * 256 + 1
    assert head[0] == 0x80000000  # row 0 begins with element 0
    # slab 1's range 0 starts with element 64, the fifth of its row 4 = child row 24; the empty ranges 1 .. 255 of slab 0 take that word
    assert set(head[1:257]) == {24}
    # everything behind takes the tail's word: element 128 lies in row 17 of slab 1 (elements 125 .. 129) = child row 37
    assert mo["tail_start"] == 37 and set(head[257:]) == {37}


def test_heads_of_a_matrix_without_tail_rows_left():
    """one row of 128 elements in one column of slab 0: tile 0 is range 0's, the tail (elements 64 .. 127) continues row 0"""
    mo = R.build_model(1, 1, [0, 128], np.zeros(128, dtype=np.int64), S=8, shift=0, value_size=8, capacity=4, min_count=2, sigma=1)
    assert mo["p"] == 2 and mo["segments"] == 1 and mo["tail_start"] == 0
    assert mo["range_head"][0] == 0x80000000 and set(mo["range_head"][1:]) == {0}
    assert list(mo["range_cost"]) == [0, 195 * 64 + 16]


def test_value_positions():
    """fp64, sigma 8: lane l holds elements 8 l .. 8 l + 7 in pieces (two doubles) q 64 + l, q = 0 .. 3"""
    pos = R.value_positions(1100, 512, 8, 3, 2)
    assert sorted(pos) == list(range(1100))
    assert [pos[i] for i in (0, 1, 2, 3, 8, 9, 511)] == [0, 1, 128, 129, 2, 3, 3 * 128 + 63 * 2 + 1]
    assert pos[512 + 10] == 512 + (1 * 64 + 1) * 2 and pos[1024 + 5] == 1029  # tile 1; the tail stays in CSR order
    pos4 = R.value_positions(1100, 512, 8, 3, 4)  # the fp32 copy: pieces of four
    assert [pos4[i] for i in (0, 3, 4, 8, 12)] == [0, 3, 256, 4, 260]


# ---- compare() on damaged copies ------------------------------------------------------------------------------------------------------------
DEVICE_KEYS = ("slab_off", "row_ptr", "col", "tile0", "hot_count", "hot_cols", "cold_base", "cold_cols", "col_hi", "col_lo", "range_cost",
               "range_begin", "range_head")


@pytest.fixture(scope="module")
def random_model():
    rng = np.random.default_rng(21)
    m, n = 300, 900
    lens = rng.integers(0, 30, size=m)
    row_ptr = np.concatenate([[0], np.cumsum(lens)])
    col = np.where(rng.random(row_ptr[-1]) < 0.7, rng.integers(0, 60, size=row_ptr[-1]) * 13 % n, rng.integers(0, n, size=row_ptr[-1]))
    mo = R.build_model(m, n, row_ptr, col, S=8, shift=2, value_size=8, capacity=8, min_count=2, sigma=1)
    assert all(s["thr"] > 2 for s in mo["selection"]) and mo["foreign_hot"].any() and mo["cold_total"] > 100
    return mo


def _copy(mo):
    dev = {k: mo[k] for k in R.SCALARS}
    dev.update({k: np.array(mo[k]) for k in DEVICE_KEYS})
    return dev


def test_an_undamaged_copy_compares_equal(random_model, two_slabs):
    assert R.compare(random_model, _copy(random_model)) == []
    assert R.compare(two_slabs, _copy(two_slabs)) == []
    assert np.array_equal(R.decode(random_model), random_model["col"][:random_model["code"].size])


def test_every_damage_is_reported_by_array_and_index(random_model):
    mo = random_model

    def report(damage):
        dev = _copy(mo)
        name, index = damage(dev)
        found = R.compare(mo, dev)
        assert [(f[0], f[1]) for f in found] == [(name, index)], found

    def flip_hot_bit(dev):
        dev["col_hi"][777] ^= 0x80
        return "col_hi", 777

    def swap_two_slots(dev):
        k = int(np.argmax(mo["hot_count"]))
        dev["hot_cols"][k, [2, 3]] = dev["hot_cols"][k, [3, 2]]
        return "hot_cols", k * mo["capacity"] + 2

    def move_one_cut(dev):
        k = int(np.argmax(np.diff(mo["tile0"])))
        rho = int(np.flatnonzero(np.diff(mo["range_begin"][k]) > 0)[1])  # the second range that has a tile: its begin moves
        dev["range_begin"][k, rho] += 1
        return "range_begin", k * 257 + rho

    def set_one_start_bit(dev):
        i = int(np.flatnonzero((mo["col_hi"] & 0x40) == 0)[50])
        dev["col_hi"][i] |= 0x40
        return "col_hi", i

    def swap_two_cold_entries(dev):
        dev["cold_cols"][[30, 31]] = dev["cold_cols"][[31, 30]]
        return "cold_cols", 30

    def clear_one_exact(dev):
        R_ = int(np.flatnonzero(mo["range_head"] & 0x80000000)[3])
        dev["range_head"][R_] &= 0x7FFFFFFF
        return "range_head", R_

    def one_slot_in_use_more(dev):
        dev["hot_count"][5] += 1
        return "hot_count", 5

    def low_half_of_one_code(dev):
        dev["col_lo"][4000] ^= 1
        return "col_lo", 4000

    def one_prefix_cost(dev):
        dev["range_cost"][9] += 16
        return "range_cost", 9

    def a_scalar(dev):
        dev["cold_total"] += 1
        return "scalars", R.SCALARS.index("cold_total")

    for damage in (flip_hot_bit, swap_two_slots, move_one_cut, set_one_start_bit, swap_two_cold_entries, clear_one_exact, one_slot_in_use_more,
                   low_half_of_one_code, one_prefix_cost, a_scalar):
        report(damage)


def test_a_shorter_array_is_reported_at_its_end(random_model):
    dev = _copy(random_model)
    dev["cold_cols"] = dev["cold_cols"][:-1]
    assert R.compare(random_model, dev) == [("cold_cols", random_model["cold_total"] - 1, random_model["cold_total"], random_model["cold_total"] - 1)]
