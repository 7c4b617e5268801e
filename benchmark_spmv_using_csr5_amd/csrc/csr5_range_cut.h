// csr5_range_cut.h -- which tiles of a slab every wavefront range of the persistent kernel (csr5_hot.hip k_spmv_range) walks.
// Plain functions over plain integers, host and device: the conversion calls them from a kernel (k_range_cuts), and they
// compile with g++ alone (scripts/host_emulation/range_cut_main.cpp, tests/test_range_cut_host.py).  No HIP include.
//
// The ranges of a slab are cut by MODELLED COST, not by tile count.  A tile's cost is known at conversion from its packed
// column codes:
//     cost(t) = A T + B min(cold(t), T / 2) + C starts(t)          (T = elements of a tile)
// cold(t) = elements of the tile that are gathered through the vector memory path (bit 23 of the code clear), starts(t) =
// elements that start a row of the child (bit 22 set).  With E[i] = cost of the slab's tiles 0 .. i-1 (E[0] = 0, E[n] = W):
//   * workgroup boundary g = 0 .. 32 of the slab is the first tile i with E[i] >= ceil(g W / 32) -- or, with spans by COUNT
//     (what the library uses, see RANGE_SPANS_BY_COUNT), the same with every tile costing 1: tile ceil(g n / 32);
//   * inside a workgroup's span [b_g, b_g+1), whose cost is V, wavefront boundary j = 0 .. 8 is the first tile i of the span
//     with E[i] - E[b_g] >= ceil(V cum_j / cum_8), cum_j = sum of the slot factors of wavefronts 0 .. j-1;
//   * boundaries never decrease, the first of a span is its first tile and the last is its end (so the first of a slab is 0
//     and the last is n, whatever the costs are).  A range may be empty.
// Integers only: the cuts are a pure function of the column codes, the same on every device and in every run.
//
// Where the constants come from: profiles/r07_range_cost.md (scripts/experiments/range_cost_fit.py: least squares of the
// wall-clock duration of the 4 096 ranges of R-MAT 24 on tiles, cold lanes, row starts and wavefront slot, checked on
// R-MAT 22 without refitting).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CSR5_CUT_HD __host__ __device__ inline
#else
#define CSR5_CUT_HD inline
#endif

namespace csr5 {

#ifndef CSR5_HOT_WAVES
#define CSR5_HOT_WAVES 8
#endif
constexpr int CUT_WORKGROUPS = 32;        // workgroups per XCD = spans per slab
constexpr int CUT_WAVES = CSR5_HOT_WAVES; // wavefronts per workgroup = ranges per span
constexpr int CUT_RANGES = CUT_WORKGROUPS * CUT_WAVES;
constexpr int CUT_TABLE_STRIDE = CUT_RANGES + 1; // range_begin[slab][0 .. 256]

// Cost of one tile per element of it (A; a tile of 512 elements: 99 840), of one cold lane (B) and of one row start (C), from
// profiles/r07_range_cost.md.  B is NEGATIVE: among the eight wavefronts of a workgroup the one whose tiles hold more cold lanes
// finishes EARLIER -- a cold lane reads slot 0 of the LDS table (one address for all of them) where a hot lane reads its own slot,
// and the cold gathers' latency is hidden behind the next tile's streams -- by 15.6 ns per lane on R-MAT 24 and 17.7 ns on R-MAT 22,
// of 3.3 / 2.9 us per tile; a row start costs 1 ns.  The fit saw tiles with a quarter to two fifths of cold lanes; beyond half a
// tile of cold lanes the cost falls no further, so it stays positive whatever the tile holds.
#ifndef CSR5_RANGE_COST_A
#define CSR5_RANGE_COST_A 195
#endif
#ifndef CSR5_RANGE_COST_B
#define CSR5_RANGE_COST_B (-262)
#endif
#ifndef CSR5_RANGE_COST_C
#define CSR5_RANGE_COST_C 16
#endif
constexpr int RANGE_COST_A = CSR5_RANGE_COST_A, RANGE_COST_B = CSR5_RANGE_COST_B, RANGE_COST_C = CSR5_RANGE_COST_C;
static_assert(RANGE_COST_A > 0 && RANGE_COST_C >= 0 && 2 * RANGE_COST_A + RANGE_COST_B > 0, "a tile's cost is positive");

// The cost above is what a wavefront pays RELATIVE TO THE OTHER SEVEN of its workgroup.  Between workgroups it does not hold: along a
// slab of R-MAT 24 it predicts 10 % between the first and the last eighth of the tiles where 0.5 % were measured (3.5 % on R-MAT 22),
// and between slabs the sign turns round (a slab with more cold lanes takes longer per tile: the compute unit as a whole waits for
// its gathers).  So the workgroups' spans are cut by tile count, as before, and only the ranges inside a span by cost; for the same
// reason the slabs are still dealt to the XCDs by tile count.  (profiles/r07_range_cost.md)
constexpr bool RANGE_SPANS_BY_COUNT = true;

// Share of a workgroup's cost that each of its wavefronts takes, per mille of the mean.  With two wavefronts per SIMD the
// one that was launched first wins every issue conflict and walks equal work 5.5 % faster (profiles/r05_probes.txt section 2):
// the first four take more.
struct RangeSlots {
    int permil[CUT_WAVES];
};
constexpr RangeSlots range_slots_default()
{
    RangeSlots s{};
    for (int w = 0; w < CUT_WAVES; w++) // (another workgroup size is an experiment build: equal shares)
        s.permil[w] = CUT_WAVES != 8 ? 1000 : (w < 4 ? 1085 : 915);
    return s;
}
constexpr RangeSlots RANGE_SLOTS_DEFAULT = range_slots_default();

// T = elements of the tile, cold and starts <= T
CSR5_CUT_HD uint64_t range_tile_cost(int T, int cold, int starts)
{
    const int counted = cold < T / 2 ? cold : T / 2;
    return (uint64_t)((int64_t)RANGE_COST_A * T + (int64_t)RANGE_COST_B * counted + (int64_t)RANGE_COST_C * starts);
}

// ceil(a * num / den) for a < 2^50, num <= den < 2^13
CSR5_CUT_HD uint64_t cut_share(uint64_t a, uint64_t num, uint64_t den) { return den ? (a * num + den - 1) / den : 0; }

// first i in [lo, hi] with E[i] - E[0] >= target, hi if there is none (E non-decreasing)
CSR5_CUT_HD int cut_first_reaching(const uint64_t *E, int lo, int hi, uint64_t target)
{
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (E[mid] - E[0] >= target)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// E: n + 1 prefix costs of the slab's tiles (only differences to E[0] are used, so a pointer into a longer prefix array
// will do).  Returns the first tile, relative to the slab, of range rho = 0 .. CUT_RANGES (rho == CUT_RANGES: n).
CSR5_CUT_HD int cut_span_begin(const uint64_t *E, int n, int g, bool by_count)
{
    if (g <= 0)
        return 0;
    if (g >= CUT_WORKGROUPS)
        return n;
    if (by_count)
        return (int)(((int64_t)g * n + CUT_WORKGROUPS - 1) / CUT_WORKGROUPS);
    return cut_first_reaching(E, 0, n, cut_share(E[n] - E[0], (uint64_t)g, CUT_WORKGROUPS));
}
CSR5_CUT_HD int range_cut_begin(const uint64_t *E, int n, int rho, const RangeSlots &slots, bool spans_by_count = RANGE_SPANS_BY_COUNT)
{
    if (rho <= 0)
        return 0;
    if (rho >= CUT_RANGES)
        return n;
    const int g = rho / CUT_WAVES, j = rho % CUT_WAVES;
    const int b0 = cut_span_begin(E, n, g, spans_by_count);
    if (j == 0)
        return b0;
    const int b1 = cut_span_begin(E, n, g + 1, spans_by_count);
    uint64_t cum = 0, all = 0;
    for (int w = 0; w < CUT_WAVES; w++) {
        cum += w < j ? (uint64_t)slots.permil[w] : 0;
        all += (uint64_t)slots.permil[w];
    }
    const uint64_t V = E[b1] - E[b0];
    return cut_first_reaching(E, b0, b1, (E[b0] - E[0]) + cut_share(V, cum, all));
}

} // namespace csr5
