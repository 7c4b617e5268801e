"""Host model of the hot slab child: every array the conversion builds for the persistent range kernel, computed from the RULE as the comments
state it (csrc/csr5_slab.hip: file header, "Every column with count >= thr ...", "One persistent pass over the child's column words ...",
"frequency order of the cold columns"; csr5_slabmap.h; csr5_slab_plan.h; csr5_range_cut.h; csr5_hot.hip: range_load, k_range_heads), not from
the kernels: numpy and Python integers, linear scans, sorts by explicit keys; no bisection, no ballots, no bitmaps.  No torch, no GPU.

build_model(m, n, row_ptr, col, S, shift, value_size, capacity, min_count) holds at stride == 1, where the sampled use counts of the table
selection are the exact ones.  compare(model, device) names every array that differs and the first index at which it does.

The rule, in the order the model follows it:
  * slab of a column = xor of all `bits`-wide groups of (col >> shift), bits = log2 S; inside a slab the columns are renumbered densely by
    dropping the lowest group (slab_local), which keeps column order.
  * the child is the stable partition of the non-zeros by slab (CSR order inside a slab); a child row (segment) starts where (slab, row) changes.
  * table of slab k: thr = smallest b >= min_count such that the columns with min(count, 2047) >= b number at most capacity - 1 (slot 0 is
    reserved); they all get a slot.  The second class -- count == thr - 1 >= min_count -- gets the room that is left, by leading buckets of
    hot_hash(c) = (c * 2654435761 mod 2^32) >> 21 for as long as the buckets' running total fits the room.  Slots are numbered from 1 in
    slab-local-id order; hot_count = slots in use, slot 0 included.
  * a tile (T = 64 sigma elements, sigma = 4096 / (64 value_size)) belongs to the slab of its first element: tile0[k] = min(ceil(slab_off[k] /
    T), p - 1).  An element is coded with its column's slot only in front of its tile's slab end; behind it the element is cold, numbered by its
    own slab.  code = 0x800000 | slot, or the column's cold rank; | 0x400000 where a child row starts.  Tiles 0 .. p-2 only (p-1 is the CSR tail).
  * cold region of slab k: the columns gathered cold somewhere, by descending min(count, 1023), ties by local id.
  * cost(t) = A T + B min(cold(t), T / 2) + C starts(t); the cuts of a slab are rule_cuts(costs of its tiles, slot factors, spans by count).
  * head of a range = child row of the first element of its first tile, | 0x80000000 when the row begins there; a range without tiles takes the
    word of the next range that has some; the CSR tail is the last "range"; 0x7FFFFFFF where nothing follows.
  * values: element l sigma + q PER + e of tile t lies in 16-byte piece q 64 + l of the tile at position e, PER = 16 / sizeof(stored type)."""
import os
import re

import numpy as np

from tests.test_range_cut_host import DEFAULT_SLOTS, rule_cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMEGA = 64
HOT_BUCKETS = 2048
COLD_COUNT_CAP = 1023
RANGES = 256
CODE_HOT, CODE_START = 0x800000, 0x400000
RANGE_EXACT, RANGE_NONE = 0x80000000, 0x7FFFFFFF
WAVE_LDS = 4096  # bytes of one wavefront's tile of values: sigma = 4096 / (64 value_size)


def cost_constants():
    """A, B, C: the #define defaults of csr5_range_cut.h"""
    text = open(os.path.join(ROOT, "benchmark_spmv_using_csr5_amd", "csrc", "csr5_range_cut.h")).read()
    return tuple(int(re.search(rf"#define CSR5_RANGE_COST_{k}\s+\(?(-?\d+)\)?", text).group(1)) for k in "ABC")


def log2_ceil(S):
    bits = 0
    while (1 << bits) < S:
        bits += 1
    return bits


def slab_of(col, shift, bits):
    v = np.asarray(col, dtype=np.int64) >> shift
    out = np.zeros_like(v)
    while np.any(v):
        out ^= v & ((1 << bits) - 1)
        v = v >> bits
    return out


def slab_local(col, shift, bits):
    col = np.asarray(col, dtype=np.int64)
    return ((col >> (shift + bits)) << shift) | (col & ((1 << shift) - 1))


def slab_local_count(n, shift, bits):
    return (((max(n, 1) - 1) >> (shift + bits)) + 1) << shift


def slab_column(k, local, shift, bits):
    """the column of slab k with that local id: the lowest group is what makes the xor of all groups equal k"""
    local = np.asarray(local, dtype=np.int64)
    hi, lo = local >> shift, local & ((1 << shift) - 1)
    low_group = k ^ slab_of(hi << shift, shift, bits)
    return (hi << (shift + bits)) | (low_group << shift) | lo


def hot_hash(col):
    return ((np.asarray(col, dtype=np.int64) * 2654435761) & 0xFFFFFFFF) >> 21


def slab_cover_pct(covered, stride, nnz):
    return min(100, covered * stride * 100 // nnz)


def select_table(cols, counts, shift, bits, capacity, min_count):
    """One slab: cols = its columns with a use, counts = their uses.  Returns (the columns with a slot in slot order, thr, the second class,
    the admitted part of it, the sizes of the class's hash buckets)."""
    capped = np.minimum(np.asarray(counts, dtype=np.int64), HOT_BUCKETS - 1)
    cols = np.asarray(cols, dtype=np.int64)
    thr = HOT_BUCKETS
    for b in range(min_count, HOT_BUCKETS + 1):
        if int(np.count_nonzero(capped >= b)) <= capacity - 1:
            thr = b
            break
    first = capped >= thr
    second = (capped == thr - 1) & (thr - 1 >= min_count)
    room = capacity - 1 - int(np.count_nonzero(first))
    buckets = np.bincount(hot_hash(cols[second]), minlength=HOT_BUCKETS)
    take, run = 0, 0
    for b in range(HOT_BUCKETS):
        run += int(buckets[b])
        if run > room:
            break
        take = b + 1
    admitted = second & (hot_hash(cols) < take)
    chosen = cols[first | admitted]
    chosen = chosen[np.argsort(slab_local(chosen, shift, bits), kind="stable")]
    return chosen, thr, cols[second], cols[admitted], buckets


def build_model(m, n, row_ptr, col, S, shift, value_size, capacity, min_count, sigma=None):
    """sigma: the child's (default: what the library takes for that value size); the host tests pass a small one to get tiles of 64 elements"""
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    nnz, bits = int(col.size), log2_ceil(S)
    sigma = sigma or WAVE_LDS // (OMEGA * value_size)
    T = OMEGA * sigma
    p = -(-nnz // T)
    A, B, C = cost_constants()
    out = dict(S=S, capacity=capacity, slab_shift=shift, slab_bits=bits, sigma=sigma, T=T, p=p, min_count=min_count, stride=1)

    # the child: stable partition by slab; a segment starts where (slab, row) changes
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(row_ptr))
    slab = slab_of(col, shift, bits)
    order = np.argsort(slab, kind="stable")
    ccol, crow, cslab = col[order], row[order], slab[order]
    start = np.ones(nnz, dtype=bool)
    start[1:] = (cslab[1:] != cslab[:-1]) | (crow[1:] != crow[:-1])
    child_ptr = np.append(np.flatnonzero(start), nnz)
    segments = child_ptr.size - 1
    slab_off = np.array([int(np.count_nonzero(cslab < k)) for k in range(S + 1)], dtype=np.int64)
    out.update(order=order, col=ccol, row_ptr=child_ptr, segments=segments, slab_off=slab_off)

    # the table of every slab
    counts = np.bincount(col, minlength=n)
    used = np.flatnonzero(counts)
    used_slab = slab_of(used, shift, bits)
    slot_of = np.zeros(n, dtype=np.int64)  # 0 = no slot
    hot_cols = np.zeros((S, capacity), dtype=np.int64)
    hot_count = np.zeros(S, dtype=np.int64)
    covered, selection = 0, []
    for k in range(S):
        mine = used[used_slab == k]
        chosen, thr, second, admitted, buckets = select_table(mine, counts[mine], shift, bits, capacity, min_count)
        assert chosen.size <= capacity - 1
        slot_of[chosen] = np.arange(1, chosen.size + 1)
        hot_cols[k, 1:chosen.size + 1] = chosen
        hot_count[k] = chosen.size + 1
        covered += int(counts[chosen].sum())
        selection.append(dict(thr=thr, second=second, admitted=admitted, buckets=buckets))
    out.update(hot_cols=hot_cols, hot_count=hot_count, covered=covered, cover_pct=slab_cover_pct(covered, 1, nnz) if nnz else 0,
               selection=selection, slot_of=slot_of)

    # tiles: owner = slab of the first element; an element is hot only in front of its tile's slab end
    tile0 = np.minimum(-(-slab_off // T), p - 1)
    body = max(p - 1, 0) * T
    pos = np.arange(body, dtype=np.int64)
    owner = cslab[(pos // T) * T]
    in_front = pos < slab_off[owner + 1]
    hot = in_front & (slot_of[ccol[:body]] > 0)
    foreign_hot = ~in_front & (slot_of[ccol[:body]] > 0)  # the column has a slot in its own slab, the tile runs with another table
    out.update(tile0=tile0, hot=hot, foreign_hot=foreign_hot)

    # cold regions: the columns gathered cold somewhere, per slab by descending min(count, 1023), ties by local id
    marked = np.unique(ccol[:body][~hot])
    marked_slab = slab_of(marked, shift, bits)
    rank_of = np.zeros(n, dtype=np.int64)
    cold_base, cold_cols = np.zeros(S + 1, dtype=np.int64), []
    for k in range(S):
        mine = marked[marked_slab == k]
        key = np.lexsort((slab_local(mine, shift, bits), -np.minimum(counts[mine], COLD_COUNT_CAP)))  # (last key is the primary one)
        mine = mine[key]
        rank_of[mine] = np.arange(mine.size)
        cold_cols.append(mine)
        cold_base[k + 1] = cold_base[k] + mine.size
    cold_cols = np.concatenate(cold_cols) if cold_cols else np.zeros(0, dtype=np.int64)
    out.update(cold_base=cold_base, cold_cols=cold_cols, cold_total=int(cold_base[S]))

    # codes
    code = np.where(hot, CODE_HOT | slot_of[ccol[:body]], rank_of[ccol[:body]]) | np.where(start[:body], CODE_START, 0)
    out.update(code=code, col_lo=(code & 0xFFFF).astype(np.uint16), col_hi=(code >> 16).astype(np.uint8))

    # tile costs from the model's own codes, prefix costs, cuts
    tiles = max(p - 1, 0)
    cold_t = ((code & CODE_HOT) == 0).reshape(tiles, T).sum(axis=1)
    starts_t = ((code & CODE_START) != 0).reshape(tiles, T).sum(axis=1)
    costs = A * T + B * np.minimum(cold_t, T // 2) + C * starts_t
    out["tile_cold"], out["tile_starts"] = cold_t, starts_t
    out["range_cost"] = np.concatenate([[0], np.cumsum(costs)]).astype(np.uint64)
    range_begin = np.zeros((S, RANGES + 1), dtype=np.int64)
    for k in range(S):
        t0, t1 = int(tile0[k]), int(tile0[k + 1])
        range_begin[k] = t0 + np.array(rule_cuts([int(c) for c in costs[t0:t1]], DEFAULT_SLOTS, by_count=True))
    out["range_begin"] = range_begin

    # heads: the child row of every element is the number of row starts up to it, minus one
    row_of = np.cumsum(start) - 1

    def head_word(first):
        return int(row_of[first]) | (RANGE_EXACT if start[first] else 0)

    tail_first = (p - 1) * T
    tail_start = int(row_of[tail_first]) if nnz > 0 else segments
    heads = [None] * (S * RANGES + 1)
    for k in range(S):
        for rho in range(RANGES):
            if range_begin[k, rho + 1] > range_begin[k, rho]:
                heads[k * RANGES + rho] = head_word(int(range_begin[k, rho]) * T)
    heads[S * RANGES] = head_word(tail_first) if tail_start < segments else None
    nxt = RANGE_NONE
    for R in range(S * RANGES, -1, -1):
        if heads[R] is None:
            heads[R] = nxt
        else:
            nxt = heads[R]
    out.update(tail_start=tail_start, range_head=np.array(heads, dtype=np.uint32))

    out["val_pos"] = {per: value_positions(nnz, T, sigma, p, per) for per in {16 // value_size, 4}}
    return out


def value_positions(nnz, T, sigma, p, per):
    """where element i of the child (CSR order) is stored: tiles 0 .. p-2 in lane-major 16-byte pieces of `per` values, the tail as it is"""
    i = np.arange(nnz, dtype=np.int64)
    t, r = i // T, i % T
    l, j = r // sigma, r % sigma
    q, e = j // per, j % per
    return np.where(t < p - 1, t * T + (q * OMEGA + l) * per + e, i)


def decode(model):
    """the column behind every code of the model (or of a device copy laid over it), through hot_cols / cold_cols"""
    code = model["col_lo"].astype(np.int64) | (model["col_hi"].astype(np.int64) << 16)
    body, T = code.size, model["T"]
    pos = np.arange(body, dtype=np.int64)
    cslab = slab_of(model["col"][:body], model["slab_shift"], model["slab_bits"])
    owner = cslab[(pos // T) * T]
    hot = (code & CODE_HOT) != 0
    low = code & 0x3FFFFF
    cold_at = np.minimum(np.asarray(model["cold_base"])[cslab] + low, max(len(model["cold_cols"]) - 1, 0))
    cold = np.asarray(model["cold_cols"])[cold_at] if len(model["cold_cols"]) else np.zeros(body, dtype=np.int64)
    return np.where(hot, np.asarray(model["hot_cols"])[owner, np.minimum(low, model["capacity"] - 1)], cold)


# what compare() holds against each other, in the order of the build; each entry: name -> (model's array, device's array)
def _pairs(model, dev):
    S, cap, body = model["S"], model["capacity"], max(model["p"] - 1, 0) * model["T"]
    in_use = np.arange(cap)[None, :] < np.asarray(model["hot_count"])[:, None]
    yield "scalars", np.array([model[k] for k in SCALARS]), np.array([dev[k] for k in SCALARS])
    yield "slab_off", model["slab_off"], dev["slab_off"]
    yield "row_ptr", model["row_ptr"], dev["row_ptr"]
    yield "col", model["col"], dev["col"]
    yield "tile0", model["tile0"], dev["tile0"]
    yield "hot_count", model["hot_count"], dev["hot_count"]
    yield "hot_cols", np.where(in_use, model["hot_cols"], -1).ravel(), np.where(in_use, np.asarray(dev["hot_cols"]).reshape(S, cap), -1).ravel()
    yield "cold_base", model["cold_base"], dev["cold_base"]
    yield "cold_cols", model["cold_cols"], dev["cold_cols"]
    yield "col_hi", model["col_hi"], np.asarray(dev["col_hi"])[:body]
    yield "col_lo", model["col_lo"], np.asarray(dev["col_lo"])[:body]
    yield "range_cost", model["range_cost"], dev["range_cost"]
    yield "range_begin", np.asarray(model["range_begin"]).ravel(), np.asarray(dev["range_begin"]).ravel()
    yield "range_head", model["range_head"], dev["range_head"]


SCALARS = ("S", "capacity", "slab_shift", "slab_bits", "sigma", "T", "p", "tail_start", "segments", "cold_total", "stride", "min_count")


def compare(model, dev):
    """[(array, first differing index, model's entry, device's entry)], empty when every array of the build is equal.  A length that differs is
    reported at the shorter length.  hot_cols is compared over the slots in use (flat index k * capacity + slot), the codes over tiles 0 .. p-2."""
    found = []
    for name, a, b in _pairs(model, dev):
        a, b = np.asarray(a), np.asarray(b)
        wide = np.uint64 if np.uint64 in (a.dtype, b.dtype) else np.int64
        a, b = a.astype(wide, copy=False), b.astype(wide, copy=False)
        n = min(a.size, b.size)
        bad = np.flatnonzero(a[:n] != b[:n])
        if bad.size:
            found.append((name, int(bad[0]), int(a[bad[0]]), int(b[bad[0]])))
        elif a.size != b.size:
            found.append((name, n, int(a.size), int(b.size)))
    return found
