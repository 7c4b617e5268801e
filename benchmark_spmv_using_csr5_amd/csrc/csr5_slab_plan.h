// csr5_slab_plan.h -- every decision of the column-slab build (csr5_slab_build.hip) as plain functions over plain structs: the
// slab count, the hot-table gates, the rule after the column sample, the layout of the build's one temporary allocation, the
// memory estimate behind CSR5HIP_OPT_SLAB_MEMORY_MIB and the dealing of slabs onto XCDs.  No HIP include: it compiles with g++
// (scripts/host_emulation/slab_plan_main.cpp, tests/test_slab_plan_host.py).  Sizes that only the device library knows come in
// as numbers (SlabTmpSizes).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "csr5hip.h"

namespace csr5 {

// What the caller asked for (csr5hip_set_option), one field per option; part of every handle (csr5_handle.h).  It lives here
// because the plan reads it.
struct Requests {
    int nt = 1;    // CSR5HIP_OPT_STREAM_NT: 0 off, 1 auto (default), 2 force
    int ldsy = 1;  // CSR5HIP_OPT_LDS_Y: 0 off, 1 auto (default), 2 force
    int xwin = 1;  // CSR5HIP_OPT_X_WINDOW: 0 off, 1 auto (default), 2 force
    int defer = 1; // CSR5HIP_OPT_DEFER_CARRIES: 0 off, 1 auto (default), 2 force
    int col16 = 1; // CSR5HIP_OPT_NARROW_COLUMNS: 0 off, 1 auto (default)
    int col31 = 1; // CSR5HIP_OPT_FLAGGED_COLUMNS: 0 off, 1 auto (default), 2 force
    int slab = 1;  // CSR5HIP_OPT_COLUMN_SLABS: 0 off, 1 auto, 2..64 = S
    int slab_shift = 4;   // CSR5HIP_OPT_SLAB_SHIFT
    int slab_mem_mib = 0; // CSR5HIP_OPT_SLAB_MEMORY_MIB: cap on the structure's device memory (0 = none)
    int hot = 1;          // CSR5HIP_OPT_SLAB_HOT: 0 off, 1 auto, 2 force
    int narrow = 0;       // CSR5HIP_OPT_NARROW_VALUES: 1 = keep the hot child's fp64 values as fp32 when every one of them is exact
    int zero_empty = 0;   // CSR5HIP_OPT_ZERO_EMPTY_ROWS
    int x_snapshot = 0;   // CSR5HIP_OPT_X_SNAPSHOT: 0 = the copy is refreshed by every spmv(), 1 = by setX only
};

// The constants the plan shares with the kernels.  csr5_internal.h owns them (it needs HIP); csr5_slab_build.hip asserts that
// the two sets agree.
#ifndef CSR5_HOT_WAVES
#define CSR5_HOT_WAVES 8
#endif
constexpr int PLAN_OMEGA = CSR5HIP_OMEGA;
constexpr int PLAN_NUM_XCD = 8;
constexpr int PLAN_HOT_LDS_BYTES = 128 * 1024;
constexpr int PLAN_HOT_WAVE_LDS = 4096;
constexpr int PLAN_HOT_WAVES = CSR5_HOT_WAVES;
constexpr int PLAN_HOT_RANGES_PER_SLAB = 32 * PLAN_HOT_WAVES;
constexpr int PLAN_HOT_AUTO_MIN_COVER_PCT = 25;
constexpr long long PLAN_HOT_AUTO_MIN_COVERED_BEYOND = 5000000;
constexpr int plan_hot_child_sigma(int value_size) { return PLAN_HOT_WAVE_LDS / (PLAN_OMEGA * value_size); }
// columns of one slab (csr5_slabmap.h slab_local_count, restated: that header is device code)
inline size_t plan_local_columns(int n, int bits, int shift)
{
    return ((size_t)(((uint32_t)(n > 0 ? n - 1 : 0)) >> (shift + bits)) + 1) << shift;
}
inline int plan_log2_ceil(int S)
{
    int bits = 0;
    while ((1 << bits) < S)
        bits++;
    return bits;
}

struct SlabInputs {
    int m, n, nnz, p, sigma, tile_elems; // the parent's geometry
    int value_size;                      // 8 (fp64) or 4
    long long xwin_covered;              // non-zeros inside the x windows found at conversion
    Requests req;
    int mode;      // SpmvOptions::mode
    bool is_child; // internal handle of a slab structure: never builds slabs itself
    int lds_max;   // the device's LDS limit per workgroup; asked only when slab_table_possible() (0: not asked)
};

struct SlabPlan {
    SlabInputs in;
    int S;        // slabs while the table stays in use (0: no structure, nothing else is set)
    int S_plain;  // the count if the table is not used
    int S_alloc;  // the larger of the two: what the temporaries are sized for
    int bits_s, bits_alloc; // log2 of S and of S_alloc
    bool auto_count;        // the count was left to the library
    bool hot;               // the LDS hot table is a candidate: the column sample decides (slab_after_sample)
    int hot_sigma, hot_T, hot_p; // sigma, tile elements and tiles of a hot child
    int hot_capacity;            // table slots per slab
    int stride, min_count;       // the column sample: one 64-element chunk in `stride`, uses a column needs for a slot
};

// The slab count by the size of x alone (auto rule):
// one slab per XCD while a slab's share of x stays within a few L2 sizes; two per XCD beyond (measured with the hot
// table on R-MAT 20 / 22 / 24, x = 8 / 34 / 134 MB: 8 slabs 73 / 329 / 1564 us, 16 slabs 85 / 357 / 1505 us, 32 slabs
// 119 / 441 / 1674 us: every further round costs a table refill and a workgroup barrier)
// (beyond R-MAT 24 -- scale 25 / 26, x = 268 / 537 MB -- four slabs per XCD win again: 3 011 vs 3 113 us, 6 691 vs 6 970 us)
inline int slab_count_by_x(long long xbytes)
{
    return xbytes < 64LL * 1024 * 1024 ? 8 : (xbytes < 256LL * 1024 * 1024 ? 16 : 32);
}

// Number of slabs spmv() should use (0 = none).  Auto rule (measured on MI355X, scripts/experiments/slab_*):
// the structure pays when x is larger than one XCD's 4-MB L2 AND the columns are scattered (the per-tile x windows
// found at conversion cover less than half of the non-zeros); a banded matrix keeps its x lines in L2 anyway and
// would only pay for the partial sums.
inline int slab_count_for(const SlabInputs &in)
{
    if (in.is_child || in.req.slab == 0 || in.p < 2 || in.nnz <= 0 || in.m <= 0)
        return 0;
    if (in.req.slab >= 2)
        return in.req.slab;
    const long long xbytes = (long long)in.n * (long long)in.value_size;
    if (xbytes < 4LL * 1024 * 1024 || in.p < 2 * 256)
        return 0;
    const long long covered_pct = in.xwin_covered * 100 / ((long long)(in.p - 1) * in.tile_elems);
    if (covered_pct >= 50)
        return 0;
    int S = slab_count_by_x(xbytes);
    // ... as long as every wavefront of the persistent kernel still gets a dozen tiles per slab (256 ranges per slab): below
    // that the pipeline restart and the table refill of every slab cost more than the coverage buys.  One of eight row
    // blocks of R-MAT 24 (25-37 M non-zeros against the full 134-MB x; 12-18 tiles per wavefront and slab at 16 slabs) is
    // faster with 16 slabs once its tables are full -- 165 / 180 / 177 us for blocks 0 / 3 / 7 against 176 / 186 / 169 with
    // 8 (scripts/experiments/shard_alone.py, profiles/r04_shards.txt).
    const long long child_tiles = (long long)in.nnz / ((long long)PLAN_OMEGA * plan_hot_child_sigma(in.value_size));
    while (S > PLAN_NUM_XCD && child_tiles / ((long long)S * PLAN_HOT_RANGES_PER_SLAB) < 12)
        S /= 2;
    return S;
}

// Slab count when the hot table is NOT used (auto mode): without the table nothing ties the count to the 8 XCDs, and
// fewer slabs mean fewer segments -- fewer partial sums to store and to combine -- as long as a slab's share of x stays
// around half an XCD's L2 (2 MiB).  webbase-like (x = 8 MB, no popular columns): 4 slabs 24.4-24.9 us, 8 slabs
// 25.4-26.1 us in the same GPU call, for every sigma.
inline int slab_count_without_table(const SlabInputs &in)
{
    const long long xbytes = (long long)in.n * (long long)in.value_size;
    int S = 2;
    while (S < 16 && (long long)S * (2LL << 20) < xbytes)
        S *= 2;
    return S;
}

// LDS hot table for the persistent kernel (fused mode, S a multiple of the 8 XCDs)?  Everything but the device's LDS limit.
// (a slab-local column id -- and with it a cold rank -- must fit the 22 bits a packed column code has for it)
inline bool slab_table_possible(const SlabInputs &in, int S)
{
    const int hot_sigma = plan_hot_child_sigma(in.value_size);
    const int hot_T = PLAN_OMEGA * hot_sigma;
    const int hot_p = (int)(((long long)in.nnz + hot_T - 1) / hot_T);
    return in.req.hot != 0 && S % PLAN_NUM_XCD == 0 && in.mode == 1 && hot_sigma >= 4 && hot_p >= 2 &&
           (long long)in.n * (long long)in.value_size <= 0x7FFFFFFFLL &&
           plan_local_columns(in.n, plan_log2_ceil(S), in.req.slab_shift) <= ((size_t)1 << 22);
}

inline SlabPlan slab_plan(const SlabInputs &in)
{
    SlabPlan pl{};
    pl.in = in;
    pl.stride = 1;
    pl.S = slab_count_for(in);
    if (!pl.S)
        return pl;
    pl.auto_count = in.req.slab == 1;
    pl.S_plain = pl.auto_count ? slab_count_without_table(in) : pl.S; // the count if the table is not used
    pl.hot_sigma = plan_hot_child_sigma(in.value_size);
    pl.hot_T = PLAN_OMEGA * pl.hot_sigma;
    pl.hot_p = (int)(((long long)in.nnz + pl.hot_T - 1) / pl.hot_T);
    pl.bits_s = plan_log2_ceil(pl.S);
    pl.hot = slab_table_possible(in, pl.S);
    if (pl.hot) {
        // the per-wavefront y-compaction regions sit behind the table (k_spmv_range)
        int lds = in.lds_max - PLAN_HOT_WAVES * PLAN_HOT_WAVE_LDS;
        lds = lds > PLAN_HOT_LDS_BYTES ? PLAN_HOT_LDS_BYTES : lds;
        pl.hot_capacity = lds / in.value_size;
        // a device (or runtime) that offers little LDS gets no table, forced or not: slot 0 is reserved and the
        // threshold search needs room above it
        if (pl.hot_capacity < 1024) {
            pl.hot = false;
            pl.hot_capacity = 0;
        }
    }
    if (!pl.hot && pl.auto_count)
        pl.S = pl.S_plain; // table ruled out beforehand
    pl.S_alloc = pl.S > pl.S_plain ? pl.S : pl.S_plain;
    pl.bits_alloc = plan_log2_ceil(pl.S_alloc);
    if (pl.hot) {
        // Column use counts come from a sample of the non-zeros (one 64-element chunk in `stride`): ~4 M samples are
        // plenty to rank columns, and a full count serialises on the very columns it is looking for.
        int stride = (int)(in.nnz / (4LL * 1024 * 1024));
        stride = stride < 1 ? 1 : (stride > 64 ? 64 : stride); // (R-MAT 24: 1/64 ranks as well as 1/32 -- also the cold regions, round 4: 1/16 and 1/8 leave the L2 misses at 30.8 M and cost 0.7 / 1.8 ms of conversion --, 1/128 costs 1.5 % of the SpMV)
        // A slot is staged by each of the 32 workgroups of the slab's XCD in every SpMV (a coalesced copy out of the
        // permuted x: about what two cold gathers cost), so a column must be used a few times per SpMV to earn one -- and
        // the sample must have seen it twice to say so.  16 uses: with 48 (round 3) a row block of R-MAT 24 -- its columns
        // are used an eighth as often -- left a quarter of its table empty (coverage 60 -> 72 %, 189 -> 180 us on the slowest
        // of the eight blocks, profiles/r04_shards.txt); the whole matrix fills its tables either way.
        int min_count = 16 / stride;
        min_count = min_count < 2 ? 2 : min_count;
        pl.stride = stride;
        pl.min_count = min_count;
    }
    return pl;
}

// share of the non-zeros whose column got a table slot, from the sample's count: an estimate
inline int slab_cover_pct(const SlabPlan &pl, unsigned long long covered)
{
    const int pct = (int)(covered * (unsigned long long)pl.stride * 100 / (unsigned long long)pl.in.nnz);
    return pct > 100 ? 100 : pct;
}

enum SlabVerdict { SLAB_NONE, SLAB_NO_TABLE, SLAB_TABLE };
struct SlabChoice {
    SlabVerdict verdict;
    int S, bits; // the final slab count and its log2 (0 with SLAB_NONE)
};

// What is built once the sample has said how much the table would cover (a plan without a candidate table: no sample, S as planned).
inline SlabChoice slab_after_sample(const SlabPlan &pl, int hot_cover_pct)
{
    int S = pl.S;
    bool hot = pl.hot;
    if (hot) {
        // Worth it when a good part of the gathers leaves the vector memory path AND the matrix is large enough to pay for the
        // persistent kernel's fixed costs (a table refill and a workgroup barrier per slab, the range seams, P + combine: a
        // 3 M-nnz matrix takes 44-49 us on this path whatever its columns).  Measured break-evens, cold (round 6,
        // scripts/experiments/round6/locality.py, profiles/r06_locality.md): R-MAT 19 (8.4 M nnz, 90 % covered) wins 13 %,
        // webbase-like x 8 with power-law columns (25 M, 54 %) wins 9 %, the same x 4 (12 M, 50 %) loses 11 %, x 2 loses 33 %, x 1
        // loses 60 %: the table pays from about 5 M non-zeros covered BEYOND the 25 % floor.
        const long long beyond = (long long)pl.in.nnz / 100 * (hot_cover_pct - PLAN_HOT_AUTO_MIN_COVER_PCT);
        hot = pl.in.req.hot == 2 || (hot_cover_pct >= PLAN_HOT_AUTO_MIN_COVER_PCT && beyond >= PLAN_HOT_AUTO_MIN_COVERED_BEYOND);
        if (!hot && pl.auto_count) {
            // Skewed columns on a matrix too small for the table: the popular part of x stays in every XCD's L2 by itself and
            // the plain kernel beats slabs without a table at every size measured (28.0 / 51.3 / 102 us against 32.2 / 56.2 /
            // 110 on webbase-like x 1 / 2 / 4 with power-law columns): no structure at all.
            if (hot_cover_pct >= PLAN_HOT_AUTO_MIN_COVER_PCT)
                return SlabChoice{SLAB_NONE, 0, 0};
            S = pl.S_plain; // the table was the reason for that slab count
        }
    }
    return SlabChoice{hot ? SLAB_TABLE : SLAB_NO_TABLE, S, plan_log2_ceil(S)};
}

// Temporary and table sizes that the device library and the slab unit own (csr5_slab.hip), asked before the layout is made.
struct SlabTmpSizes {
    size_t scan;       // slab_scan_tmp_bytes(S_alloc * p)
    size_t select;     // slab_select_tmp_bytes(nnz)
    size_t hotmap;     // slab_hotmap_bytes(n, S_alloc, bits_alloc, shift)
    int hot_buckets;   // slab_hot_buckets()
    size_t cold_words; // with a candidate table: slab_cold_words(n, S, bits_s, shift); else 0
    size_t cold_sort;  // with a candidate table: slab_cold_sort_tmp_bytes(cold_words, bits_s); else 0
    size_t base_words; // slab_base_words(m, S_alloc) (the memory estimate)
};

// all temporaries of the build in one allocation: 256-aligned regions, in this order
enum SlabRegion {
    T_HIST, T_SCAN, T_KEY, T_COUNT, T_SEL, T_CNT, T_HOTMAP, T_CHIST, T_THR,
    // ranking of the cold columns behind the packed codes (slab_hot_pack): counts / ranks, sort keys in and out, sources
    T_REF, T_RANK, T_KEYS, T_KEYS2, T_SRC, T_SORT,
    T_REGIONS
};
struct SlabArena {
    size_t off[T_REGIONS], bytes[T_REGIONS];
    size_t total;
    size_t covered() const { return off[T_COUNT] + 8; } // the sample's 8-byte count shares the segment counter's region
};

inline SlabArena slab_arena(const SlabPlan &pl, const SlabTmpSizes &sz)
{
    const SlabInputs &in = pl.in;
    SlabArena a{};
    a.bytes[T_HIST] = (size_t)pl.S_alloc * in.p * 4;
    a.bytes[T_SCAN] = sz.scan;
    a.bytes[T_KEY] = (size_t)in.nnz * 4;
    a.bytes[T_COUNT] = 16;
    a.bytes[T_SEL] = sz.select;
    a.bytes[T_CNT] = (size_t)(in.n > 0 ? in.n : 1) * 4;
    a.bytes[T_HOTMAP] = sz.hotmap;
    a.bytes[T_CHIST] = (size_t)pl.S_alloc * sz.hot_buckets * 4;
    a.bytes[T_THR] = (size_t)pl.S_alloc * 8;
    a.bytes[T_REF] = sz.cold_words;
    a.bytes[T_RANK] = a.bytes[T_KEYS] = a.bytes[T_KEYS2] = a.bytes[T_SRC] = sz.cold_words * 4;
    a.bytes[T_SORT] = sz.cold_sort;
    size_t off = 0;
    for (int r = 0; r < T_REGIONS; r++) {
        a.off[r] = off;
        off += (a.bytes[r] + 255) & ~(size_t)255;
    }
    a.total = off;
    return a;
}

// Upper bound of what the structure holds: the second copy of column_index / value (+ 3-byte column codes with a
// hot table), the build temporaries, one partial sum / row byte / child row pointer per (row, slab) segment --
// at most min(nnz, m * S) of them --, the combine's tables, the child's own conversion arena (descriptor word per
// 64 sigma elements, tile_ptr, carry state: ~300 B per child tile) and, with a hot table, the table columns, the
// wavefront-range words and the permuted copy of x with its column lists.
inline unsigned long long slab_memory_need(const SlabPlan &pl, const SlabTmpSizes &sz, size_t arena_total)
{
    const SlabInputs &in = pl.in;
    const unsigned long long vs = (unsigned long long)in.value_size;
    const unsigned long long seg_max = std::min<unsigned long long>((unsigned long long)in.nnz, (unsigned long long)in.m * pl.S_alloc);
    const unsigned long long child_tiles = (unsigned long long)in.nnz / ((unsigned long long)PLAN_OMEGA * (pl.hot ? pl.hot_sigma : in.sigma)) + 2;
    unsigned long long need = (unsigned long long)in.nnz * (4 + vs + (pl.hot ? 3 : 0)) + arena_total + seg_max * (vs + 5) +
                              sz.base_words * 4ull + (unsigned long long)in.m / 8 + child_tiles * 300ull;
    if (pl.hot && in.req.narrow && in.value_size == 8)
        need += (unsigned long long)in.nnz * 4ull; // the fp32 copy of the child's values
    if (pl.hot)
        need += (unsigned long long)pl.S * pl.hot_capacity * (4 + vs) + (unsigned long long)pl.S * PLAN_HOT_RANGES_PER_SLAB * (vs + 4) +
                std::min<unsigned long long>(sz.cold_words, (unsigned long long)in.nnz) * (4 + vs);
    return need;
}
// CSR5HIP_OPT_SLAB_MEMORY_MIB (> 0): the estimate against the cap
inline bool slab_memory_fits(unsigned long long need, int cap_mib) { return !(need > (unsigned long long)cap_mib << 20); }

// Which slabs an XCD walks.  Slabs differ in size (hub columns: the 16 slabs of R-MAT 24 span 0.86 .. 1.16 of the
// mean, and two consecutive ones still 1.12) and the kernel ends with its slowest XCD, so the slabs are dealt
// longest first onto the XCD with the least work that still has a round free.
// first_tile: S + 1 entries, the first tile of every slab; the result: the slabs of XCD 0 (one per round), of XCD 1, ...
inline std::vector<int> slab_deal(const std::vector<int32_t> &first_tile, int S)
{
    const int rounds = S / PLAN_NUM_XCD;
    std::vector<int> by_size((size_t)S), order((size_t)S, 0), used(PLAN_NUM_XCD, 0);
    std::vector<long long> load(PLAN_NUM_XCD, 0);
    for (int k = 0; k < S; k++)
        by_size[k] = k;
    std::stable_sort(by_size.begin(), by_size.end(), [&](int a, int b) {
        return first_tile[a + 1] - first_tile[a] > first_tile[b + 1] - first_tile[b];
    });
    for (int k : by_size) {
        int best = -1;
        for (int x = 0; x < PLAN_NUM_XCD; x++)
            if (used[x] < rounds && (best < 0 || load[x] < load[best]))
                best = x;
        order[(size_t)best * rounds + used[best]++] = k;
        load[best] += first_tile[k + 1] - first_tile[k];
    }
    return order;
}

} // namespace csr5
