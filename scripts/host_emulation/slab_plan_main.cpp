// slab_plan_main.cpp -- the decisions of the column-slab build (csr5_slab_plan.h) on a table of cases, one line per case.
// Plain host code, no GPU and no HIP: g++ -fsanitize=address,undefined; tests/test_slab_plan_host.py compares every line
// with a literal.
#include <cstdio>
#include <string>
#include <vector>

#include "csr5_slab_plan.h"
#include "csr5hip.h"

using namespace csr5;

static const int LDS_MI355X = 160 * 1024; // what the device reports per workgroup

// a square matrix of n columns and nnz non-zeros, converted at sigma 16, no x windows, every request at its default
static SlabInputs matrix(long long n, long long nnz, int value_size)
{
    SlabInputs in{};
    in.m = in.n = (int)n;
    in.nnz = (int)nnz;
    in.sigma = 16;
    in.tile_elems = PLAN_OMEGA * in.sigma;
    in.p = (int)((nnz + in.tile_elems - 1) / in.tile_elems);
    in.value_size = value_size;
    in.mode = 1;
    in.lds_max = LDS_MI355X;
    return in;
}

static void count(const char *name, const SlabInputs &in)
{
    printf("%s: by_x=%d count=%d\n", name, slab_count_by_x((long long)in.n * in.value_size), slab_count_for(in));
}

static void plan(const char *name, const SlabInputs &in)
{
    const SlabPlan pl = slab_plan(in);
    printf("%s: S=%d S_plain=%d S_alloc=%d bits_s=%d bits_alloc=%d auto=%d hot=%d hot_sigma=%d hot_T=%d hot_p=%d capacity=%d stride=%d "
           "min_count=%d\n",
           name, pl.S, pl.S_plain, pl.S_alloc, pl.bits_s, pl.bits_alloc, (int)pl.auto_count, (int)pl.hot, pl.hot_sigma, pl.hot_T, pl.hot_p,
           pl.hot_capacity, pl.stride, pl.min_count);
}

static void after(const char *name, const SlabInputs &in, int pct)
{
    const SlabPlan pl = slab_plan(in);
    const SlabChoice c = slab_after_sample(pl, pct);
    static const char *const verdict[] = {"none", "no_table", "table"};
    printf("%s: planned S=%d hot=%d cover=%d -> %s S=%d bits=%d\n", name, pl.S, (int)pl.hot, pct, verdict[c.verdict], c.S, c.bits);
}

// sizes as the device library might give them: odd on purpose, so that the rounding shows
static SlabTmpSizes sizes(const SlabPlan &pl)
{
    SlabTmpSizes sz{};
    sz.scan = 1031;
    sz.select = 70001;
    sz.hotmap = (size_t)pl.S_alloc * 18 * 1000 + 256;
    sz.hot_buckets = 1024;
    sz.cold_words = pl.hot ? (size_t)pl.S * plan_local_columns(pl.in.n, pl.bits_s, pl.in.req.slab_shift) : 0;
    sz.cold_sort = pl.hot ? 12345 : 0;
    sz.base_words = (size_t)(pl.in.m / 64 + 2) * pl.S_alloc;
    return sz;
}

static void arena(const char *name, const SlabInputs &in)
{
    const SlabPlan pl = slab_plan(in);
    const SlabTmpSizes sz = sizes(pl);
    const SlabArena a = slab_arena(pl, sz);
    bool aligned = a.total % 256 == 0, disjoint = true, cold_empty = true;
    printf("%s: hot=%d off", name, (int)pl.hot);
    for (int r = 0; r < T_REGIONS; r++) {
        printf(" %zu+%zu", a.off[r], a.bytes[r]);
        aligned = aligned && a.off[r] % 256 == 0;
        const size_t end = r + 1 < T_REGIONS ? a.off[r + 1] : a.total;
        disjoint = disjoint && a.off[r] + a.bytes[r] <= end;
        if (r >= T_REF)
            cold_empty = cold_empty && a.bytes[r] == 0;
    }
    printf(" total=%zu aligned=%d disjoint=%d covered_in_count=%d cold_empty=%d\n", a.total, (int)aligned, (int)disjoint,
           (int)(a.covered() == a.off[T_COUNT] + 8 && a.covered() + 8 <= a.off[T_COUNT] + a.bytes[T_COUNT]), (int)cold_empty);
}

static void memory(const char *name, const SlabInputs &in)
{
    const SlabPlan pl = slab_plan(in);
    const SlabTmpSizes sz = sizes(pl);
    const unsigned long long need = slab_memory_need(pl, sz, slab_arena(pl, sz).total);
    const int cap = (int)((need + (1ull << 20) - 1) >> 20); // the smallest cap in MiB that holds the need
    printf("%s: hot=%d need=%llu cap=%d fits=%d cap=%d fits=%d\n", name, (int)pl.hot, need, cap, (int)slab_memory_fits(need, cap), cap - 1,
           (int)slab_memory_fits(need, cap - 1));
}

static void deal(const char *name, const std::vector<int> &tiles)
{
    const int S = (int)tiles.size();
    std::vector<int32_t> first_tile((size_t)S + 1, 0);
    for (int k = 0; k < S; k++)
        first_tile[k + 1] = first_tile[k] + tiles[k];
    const std::vector<int> order = slab_deal(first_tile, S);
    std::vector<int> seen((size_t)S, 0);
    bool perm = (int)order.size() == S;
    for (int k : order)
        perm = perm && k >= 0 && k < S && !seen[k]++;
    printf("%s: order", name);
    for (int k : order)
        printf(" %d", k);
    printf(" permutation=%d per_xcd=%d\n", (int)perm, (int)order.size() / PLAN_NUM_XCD);
}

int main()
{
    const long long Mi = 1 << 20;
    // ---- gates of the auto rule, each with its neighbour: x = 8 MB, 16 M non-zeros, 16 384 tiles
    const SlabInputs base = matrix(Mi, 16 * Mi, 8);
    SlabInputs in = base;
    count("gate/base", in);
    in.is_child = true;
    count("gate/child", in);
    in = base, in.req.slab = 0;
    count("gate/request0", in);
    in = base, in.req.slab = 2, in.p = 1;
    count("gate/p1_forced", in);
    in.p = 2;
    count("gate/p2_forced", in);
    in = base, in.req.slab = 2, in.nnz = 0;
    count("gate/nnz0_forced", in);
    in.nnz = 1;
    count("gate/nnz1_forced", in);
    in = base, in.n = 524287; // fp64: 8 bytes under 4 MiB
    count("gate/x_under_4MiB_f64", in);
    in.n = 524288;
    count("gate/x_4MiB_f64", in);
    in = base, in.n = 4 * (int)Mi - 1, in.value_size = 1; // (no such value type: the only way to one byte under)
    count("gate/x_one_byte_under_4MiB", in);
    in.n = 4 * (int)Mi;
    count("gate/x_4MiB_bytes", in);
    in = base, in.p = 511;
    count("gate/p511", in);
    in.p = 512;
    count("gate/p512", in);
    in = base, in.xwin_covered = (long long)(in.p - 1) * in.tile_elems / 2;
    count("gate/window50", in);
    in.xwin_covered -= 1;
    count("gate/window49", in);

    // ---- size classes: x of 8, 34, 134, 268 and 537 MB, R-MAT-like nnz = 16 n (fp32 at 537 MB: nnz capped at 2^31 - 1)
    for (int vs : {8, 4})
        for (int scale : {20, 22, 24, 25, 26}) {
            const long long n = (1LL << scale) * (8 / vs), nnz = std::min<long long>(16 * n, 0x7FFFFFFFLL);
            const std::string name = std::string("size/") + (vs == 8 ? "f64" : "f32") + "_x" + std::to_string(n * vs / 1000000) + "MB";
            count(name.c_str(), matrix(n, nnz, vs));
        }
    count("size/halves_twice", matrix(1LL << 25, 20000000, 8)); // 32 -> 16 -> 8
    count("size/stops_at_8", matrix(1LL << 24, 5000000, 8));    // 16 -> 8 with 4 tiles per range: no further
    count("size/halves_once", matrix(1LL << 25, 30000000, 8));  // 32 -> 16

    // ---- the count without the table: x = 1, 4, 8 (webbase-like: 4), 32, 64 MiB
    for (int mib : {1, 4, 8, 32, 64})
        printf("plain/x%dMiB: S=%d\n", mib, slab_count_without_table(matrix(mib * Mi / 8, 16 * Mi, 8)));

    // ---- table candidacy
    plan("table/base_auto", base);
    in = base, in.req.slab = 8;
    plan("table/forced8", in);
    in.req.slab = 4;
    plan("table/S4_not_multiple_of_8", in);
    in = base, in.mode = 0;
    plan("table/mode0_auto", in);
    in.req.slab = 16;
    plan("table/mode0_forced16", in);
    in = base, in.req.hot = 0;
    plan("table/hot_request0", in);
    in = matrix(4096, 512, 8), in.sigma = 4, in.tile_elems = 256, in.p = 2, in.req.slab = 8;
    plan("table/hot_p1", in);
    in.nnz = 513, in.p = 3;
    plan("table/hot_p2", in);
    in = base, in.lds_max = 8 * 4096 + 1023 * 8;
    plan("table/lds_1023_slots", in);
    in.lds_max = 8 * 4096 + 1024 * 8;
    plan("table/lds_1024_slots", in);
    in = base, in.lds_max = 64 * 1024;
    plan("table/lds_64KiB", in);
    in = base, in.value_size = 4;
    plan("table/f32", in);
    in = matrix(40000000, 16 * Mi, 4), in.req.slab = 8; // 5 000 000 local columns per slab
    plan("table/local_columns_over_2^22", in);
    in = matrix(1LL << 25, 16 * Mi, 4), in.req.slab = 8; // 2^22 exactly
    plan("table/local_columns_2^22", in);
    in = matrix(300000000, 16 * Mi, 8), in.req.slab = 8; // x of 2.4 GB: beyond 32-bit byte offsets
    plan("table/x_over_2GiB", in);
    in = matrix(1LL << 24, 256 * Mi, 8);
    plan("table/rmat24_auto", in);

    // ---- after the sample.  100 M non-zeros, x = 134 MB, count left to the library
    in = matrix(1LL << 24, 100000000, 8);
    after("sample/100M_cover24", in, 24);
    after("sample/100M_cover25", in, 25);
    // ADVICE.md's cliff: 28 % of 100 M non-zeros covered and no structure at all, with no bound on the size.  The finding is
    // still open; this pins what the library does today.
    after("sample/100M_cover28", in, 28);
    after("sample/100M_cover29", in, 29);
    after("sample/100M_cover30", in, 30);
    // 25 M non-zeros, 54 % covered (webbase-like x 8 with power-law columns): keeps the table
    in = matrix(8000000, 25000000, 8);
    after("sample/25M_cover54", in, 54);
    after("sample/25M_cover44", in, 44);
    in.req.hot = 2;
    after("sample/25M_cover10_forced_table", in, 10);
    in.req.hot = 1, in.req.slab = 8;
    after("sample/25M_cover10_forced_count", in, 10);
    after("sample/25M_cover28_forced_count", in, 28);
    after("sample/25M_cover54_forced_count", in, 54);
    in.mode = 0;
    after("sample/25M_no_candidate", in, 0);

    // ---- the column sample
    for (long long nnz : {1000000LL, 4 * Mi, 8 * Mi, 4 * Mi * 16, 0x7FFFFFFFLL}) {
        in = matrix(1LL << 24, nnz, 8), in.req.slab = 8;
        plan(("stride/nnz" + std::to_string(nnz)).c_str(), in);
    }
    {
        const SlabPlan pl = slab_plan(matrix(1LL << 24, 256 * Mi, 8));
        printf("cover/rmat24: stride=%d covered=3000000 -> %d covered=5000000 -> %d\n", pl.stride, slab_cover_pct(pl, 3000000),
               slab_cover_pct(pl, 5000000));
    }

    // ---- the temporaries' arena and the memory estimate: with a candidate table and without
    in = matrix(1LL << 20, 16 * Mi, 8);
    arena("arena/table", in);
    memory("memory/table", in);
    in.req.narrow = 1;
    memory("memory/table_narrow", in);
    in = matrix(1LL << 20, 16 * Mi, 8), in.req.hot = 0;
    arena("arena/no_table", in);
    memory("memory/no_table", in);
    in = matrix(1000003, 3000017, 4), in.req.slab = 16;
    arena("arena/odd_f32", in);
    memory("memory/odd_f32", in);

    // ---- dealing slabs onto the XCDs
    deal("deal/S8", {100, 90, 120, 80, 110, 95, 105, 85});
    // the 16 slabs of R-MAT 24 span 0.86 .. 1.16 of the mean
    deal("deal/S16_rmat24", {1160, 1040, 980, 1120, 900, 1000, 860, 1080, 940, 1100, 960, 1020, 880, 1140, 920, 1060});
    {
        std::vector<int> ties(64);
        for (int k = 0; k < 64; k++)
            ties[k] = 100 + 10 * (k % 4); // sixteen slabs of each size: the stable order decides among them
        deal("deal/S64_ties", ties);
    }
    return 0;
}
