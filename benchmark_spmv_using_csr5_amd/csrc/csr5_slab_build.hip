// csr5_slab_build.hip -- builds the column-slab structure of a converted handle (kernels: csr5_slab.hip, csr5_hot.hip).  Host code
// only.  Every decision comes from csr5_slab_plan.h; this unit asks the device what the plan needs to know, then runs the phases in
// order: reserve the temporaries, select the hot columns, partition, deal and pack, convert the child, narrow the values.
#include <algorithm>
#include <string>
#include <vector>

#include "csr5_handle.h"

using namespace csr5;

static_assert(PLAN_OMEGA == OMEGA && PLAN_NUM_XCD == NUM_XCD && PLAN_HOT_LDS_BYTES == HOT_LDS_BYTES && PLAN_HOT_WAVE_LDS == HOT_WAVE_LDS &&
                  PLAN_HOT_WAVES == HOT_WAVES && PLAN_HOT_RANGES_PER_SLAB == HOT_RANGES_PER_SLAB &&
                  PLAN_HOT_AUTO_MIN_COVER_PCT == HOT_AUTO_MIN_COVER_PCT && PLAN_HOT_AUTO_MIN_COVERED_BEYOND == HOT_AUTO_MIN_COVERED_BEYOND &&
                  plan_hot_child_sigma(8) == hot_child_sigma(8) && plan_hot_child_sigma(4) == hot_child_sigma(4),
              "csr5_slab_plan.h restates constants of csr5_internal.h: keep them equal");

namespace csr5 {

void SlabStructure::release()
{
    if (child) {
        csr5hip_free(child);
        child = nullptr;
    }
    values_narrowed = false;
    refresh_map_valid = false;
    for (Buffer &b : buf)
        b.release();
    S = 0;
    m2 = 0;
    hot_cover_pct = 0;
}

void SlabStructure::deactivate()
{
    if (child) {
        child->drop_graphs();
        child->format = -1;
        child->hot_enabled = false;
    }
    S = 0;
    m2 = 0;
    hot_cover_pct = 0;
    refresh_map_valid = false; // (the next structure may partition other columns: the map is rebuilt by the next update)
}

long long SlabStructure::bytes() const
{
    long long sum = child ? (long long)child->b_arena.cap : 0;
    for (const Buffer &b : buf)
        sum += (long long)b.cap;
    return sum;
}

} // namespace csr5

namespace {

// what the phases of one build hand on
struct SlabBuild {
    csr5hip_handle h;
    SlabPlan plan;
    SlabTmpSizes sz;
    SlabArena arena;
    size_t tmp_keep;   // SLAB_TMP_KEEP
    SlabChoice choice; // after the column sample: table or not, the final slab count
    unsigned int m2;   // (row, slab) segments: the child's rows
    void *tmp(SlabRegion r) const { return (char *)h->slab[B_TMP].ptr + arena.off[r]; }
    void *covered() const { return (char *)h->slab[B_TMP].ptr + arena.covered(); }
};

// the plan, from the handle and -- only where a table is possible at all -- the device's LDS limit
int plan_slabs(csr5hip_handle h, SlabPlan *plan)
{
    SlabInputs in{};
    in.m = h->g.m, in.n = h->g.n, in.nnz = h->g.nnz, in.p = h->g.p, in.sigma = h->g.sigma, in.tile_elems = h->g.tile_elems;
    in.value_size = (int)h->vsize();
    in.xwin_covered = h->xwin_covered;
    in.req = h->req;
    in.mode = h->opt.mode;
    in.is_child = h->is_child;
    const int S = slab_count_for(in);
    if (S && slab_table_possible(in, S)) {
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        HIP_TRY(hipDeviceGetAttribute(&in.lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    }
    *plan = slab_plan(in);
    return CSR5HIP_SUCCESS;
}

// all temporaries of the build in one allocation.  Up to 1/64 of the device memory (4.5 GB of 288) they stay with
// the handle between conversions: giving 2 GB back and asking for it again cost 120-170 ms per reconversion of
// R-MAT 24 until the runtime's pool had settled, ten times the 16 ms the conversion itself takes.
int reserve_temporaries(SlabBuild &b)
{
    csr5hip_handle h = b.h;
    const Geometry &g = h->g;
    const SlabPlan &pl = b.plan;
    // (the device's total memory, asked once per handle: hipMemGetInfo walks the allocator -- a visible share of the 0.5-ms
    //  conversion of a 3 M-nnz matrix when it ran in every build)
    if (!h->device_total_bytes) {
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        h->device_total_bytes = total_b ? total_b : 1;
    }
    b.tmp_keep = std::max((size_t)64 << 20, h->device_total_bytes / 64);
    SlabTmpSizes &sz = b.sz;
    HIP_TRY(slab_scan_tmp_bytes((size_t)pl.S_alloc * g.p, &sz.scan));
    HIP_TRY(slab_select_tmp_bytes(g.nnz, &sz.select));
    sz.hot_buckets = slab_hot_buckets();
    sz.hotmap = slab_hotmap_bytes(g.n, pl.S_alloc, pl.bits_alloc, h->req.slab_shift);
    if (pl.hot) { // (S keeps this value while the table stays in use: bits_s = log2 S)
        sz.cold_words = slab_cold_words(g.n, pl.S, pl.bits_s, h->req.slab_shift);
        HIP_TRY(slab_cold_sort_tmp_bytes(sz.cold_words, pl.bits_s, &sz.cold_sort));
    }
    sz.base_words = slab_base_words(g.m, pl.S_alloc);
    b.arena = slab_arena(pl, sz);
    if (h->req.slab_mem_mib > 0 && !slab_memory_fits(slab_memory_need(pl, sz, b.arena.total), h->req.slab_mem_mib))
        return fail_hip(hipErrorOutOfMemory, "column slabs: CSR5HIP_OPT_SLAB_MEMORY_MIB");
    HIP_TRY(h->slab[B_TMP].reserve(b.arena.total));
    return CSR5HIP_SUCCESS;
}

// Hot columns FIRST: the selection needs only the column indices (the parent's array, any order), and its verdict
// decides the slab count -- without a table fewer slabs are better, and the partition then runs once.
// Leaves the sample's estimate in slab.hot_cover_pct.
int select_hot_columns(SlabBuild &b)
{
    csr5hip_handle h = b.h;
    SlabStructure &sl = h->slab;
    const Geometry &g = h->g;
    const SlabPlan &pl = b.plan;
    hipStream_t s = h->stream;
    const int S = pl.S, shift = h->req.slab_shift;
    HIP_TRY(sl[B_HOT_COLS].reserve((size_t)S * pl.hot_capacity * 4));
    HIP_TRY(sl[B_HOT_COUNT].reserve((size_t)S * 4));
    HIP_TRY(sl[B_HOT_TILE0].reserve(((size_t)2 * S + 1) * 4)); // tile0[S + 1], then the slab order of the XCDs [S]
    HIP_TRY(sl[B_SLAB_OFF].reserve(((size_t)S + 1) * 4));
    HIP_TRY(sl[B_LEAD].reserve((size_t)S * HOT_RANGES_PER_SLAB * h->vsize())); // one leading partial per wavefront range
    HIP_TRY(sl[B_RANGE_HEAD].reserve(((size_t)S * HOT_RANGES_PER_SLAB + 1) * 4));
    HIP_TRY(hipMemsetAsync(b.tmp(T_CNT), 0, b.arena.bytes[T_CNT], s));
    HIP_TRY(hipMemsetAsync(b.tmp(T_HOTMAP), 0, slab_hotmap_bytes(g.n, S, pl.bits_s, shift), s));
    HIP_TRY(hipMemsetAsync(b.tmp(T_CHIST), 0, (size_t)S * slab_hot_buckets() * 4, s));
    HIP_TRY(hipMemsetAsync(b.covered(), 0, 8, s));
    HIP_TRY(hipMemsetAsync(sl[B_HOT_COLS].ptr, 0, (size_t)S * pl.hot_capacity * 4, s));
    HIP_TRY(slab_hot_select(g.n, g.nnz, S, pl.bits_s, shift, pl.hot_capacity, pl.min_count, pl.stride, (const int32_t *)h->d.col,
                            (uint32_t *)b.tmp(T_CNT), b.tmp(T_HOTMAP), (uint32_t *)b.tmp(T_CHIST), (uint32_t *)b.tmp(T_THR),
                            (int32_t *)sl[B_HOT_COLS].ptr, (int32_t *)sl[B_HOT_COUNT].ptr, (unsigned long long *)b.covered(), s));
    unsigned long long covered = 0;
    HIP_TRY(hipMemcpyAsync(&covered, b.covered(), 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    sl.hot_cover_pct = slab_cover_pct(pl, covered);
    return CSR5HIP_SUCCESS;
}

// the stacked matrix's CSR arrays (rows = (row, slab) segments) and the combine's tables; leaves the segment count in b.m2
int partition_segments(SlabBuild &b)
{
    csr5hip_handle h = b.h;
    SlabStructure &sl = h->slab;
    const Geometry &g = h->g;
    hipStream_t s = h->stream;
    const int S = b.choice.S;
    const uint32_t *key = (const uint32_t *)b.tmp(T_KEY), *hist = (const uint32_t *)b.tmp(T_HIST);
    HIP_TRY(sl[B_COL2].reserve((size_t)g.nnz * 4));
    HIP_TRY(sl[B_VAL2].reserve((size_t)g.nnz * h->vsize()));
    HIP_TRY(slab_partition(g, h->d, h->value_type, S, b.choice.bits, h->req.slab_shift, (uint32_t *)b.tmp(T_HIST), b.tmp(T_SCAN), b.sz.scan,
                           (int32_t *)sl[B_COL2].ptr, sl[B_VAL2].ptr, (uint32_t *)b.tmp(T_KEY), s));
    HIP_TRY(slab_count_segments(g.nnz, key, b.tmp(T_SEL), (unsigned int *)b.tmp(T_COUNT), s));
    unsigned int m2 = 0;
    HIP_TRY(hipMemcpyAsync(&m2, b.tmp(T_COUNT), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    b.m2 = m2;
    HIP_TRY(sl[B_ROW_PTR2].reserve(((size_t)m2 + 1) * 4));
    HIP_TRY(sl[B_ROWIDX].reserve((size_t)m2 + 1));
    HIP_TRY(slab_segments(g.nnz, key, b.tmp(T_SEL), (int32_t *)sl[B_ROW_PTR2].ptr, (unsigned char *)sl[B_ROWIDX].ptr, s));
    HIP_TRY(sl[B_BASE].reserve(slab_base_words(g.m, S) * 4));
    HIP_TRY(sl[B_NONEMPTY].reserve(((size_t)g.m / 32 + 16) * 4));
    HIP_TRY(slab_tables(g.m, (int)m2, g.nnz, S, g.p, h->d.row_ptr, (int32_t *)sl[B_ROW_PTR2].ptr, key, hist, (uint32_t *)sl[B_BASE].ptr,
                        (uint32_t *)sl[B_NONEMPTY].ptr, s));
    HIP_TRY(sl[B_P].reserve(((size_t)m2 + 1) * h->vsize()));
    HIP_TRY(hipMemsetAsync(sl[B_P].ptr, 0, ((size_t)m2 + 1) * h->vsize(), s));
    return CSR5HIP_SUCCESS;
}

// with a table: the slabs dealt onto the XCDs (slab_deal), then the 3-byte column codes next to the plain words (the child's sigma
// is a multiple of four: whole dwords per lane) and the cold regions of the permuted x, then the cut table of the range kernel
int deal_and_pack(SlabBuild &b)
{
    csr5hip_handle h = b.h;
    SlabStructure &sl = h->slab;
    const Geometry &g = h->g;
    const SlabPlan &pl = b.plan;
    hipStream_t s = h->stream;
    const int S = b.choice.S;
    HIP_TRY(slab_hot_finish(S, g.p, pl.hot_p, pl.hot_T, g.nnz, pl.hot_capacity, (const uint32_t *)b.tmp(T_HIST), (int32_t *)sl[B_HOT_COUNT].ptr,
                            (int32_t *)sl[B_HOT_TILE0].ptr, (int32_t *)sl[B_SLAB_OFF].ptr, s));
    std::vector<int32_t> first_tile((size_t)S + 1);
    HIP_TRY(hipMemcpyAsync(first_tile.data(), sl[B_HOT_TILE0].ptr, ((size_t)S + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const std::vector<int> order = slab_deal(first_tile, S);
    HIP_TRY(hipMemcpyAsync((int32_t *)sl[B_HOT_TILE0].ptr + S + 1, order.data(), (size_t)S * 4, hipMemcpyHostToDevice, s));
    int32_t cold_total = 0;
    HIP_TRY(sl[B_COL_LO].reserve((size_t)g.nnz * 2 + 64));
    HIP_TRY(sl[B_COL_HI].reserve((size_t)g.nnz + 64));
    // the cold region holds at most one entry per column of every slab, and no more than there are non-zeros
    const size_t cold_cap = std::min(b.sz.cold_words, (size_t)g.nnz);
    HIP_TRY(sl[B_COLD_BASE].reserve(((size_t)S + 1) * 4));
    HIP_TRY(sl[B_COLD_COLS].reserve((cold_cap + 1) * 4));
    HIP_TRY(sl[B_XPERM].reserve(((size_t)S * pl.hot_capacity + cold_cap + (size_t)pl.hot_T + 1) * h->vsize())); // (+ the x entries of the child's CSR tail)
    HIP_TRY(hipMemsetAsync(b.tmp(T_REF), 0, b.sz.cold_words, s));
    HIP_TRY(slab_hot_pack(g.n, g.nnz, pl.hot_T, pl.hot_p, S, b.choice.bits, h->req.slab_shift, (const int32_t *)sl[B_SLAB_OFF].ptr,
                          b.tmp(T_HOTMAP), (const uint32_t *)b.tmp(T_CNT), (const uint32_t *)b.tmp(T_KEY), (int32_t *)sl[B_COL2].ptr,
                          (uint16_t *)sl[B_COL_LO].ptr, (uint8_t *)sl[B_COL_HI].ptr, (uint8_t *)b.tmp(T_REF), (uint32_t *)b.tmp(T_RANK),
                          (uint32_t *)b.tmp(T_KEYS), (uint32_t *)b.tmp(T_KEYS2), (uint32_t *)b.tmp(T_SRC), b.tmp(T_SORT), b.sz.cold_sort,
                          (int32_t *)sl[B_COLD_BASE].ptr, (int32_t *)sl[B_COLD_COLS].ptr, s));
    // the codes say what every tile costs a wavefront next to the others of its workgroup (cold lanes, row starts): every workgroup's
    // span of a slab is cut into its wavefronts' ranges by that cost (csr5_range_cut.h)
    const int tiles = pl.hot_p - 1;
    HIP_TRY(sl[B_RANGE_CUT].reserve(range_cut_layout(S, tiles).total));
    HIP_TRY(launch_range_cuts(S, tiles, pl.hot_T, (const int32_t *)sl[B_HOT_TILE0].ptr, (const uint8_t *)sl[B_COL_HI].ptr, sl[B_RANGE_CUT].ptr, s));
    HIP_TRY(hipMemcpyAsync(&cold_total, (int32_t *)sl[B_COLD_BASE].ptr + S, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // (`order` is in use until here)
    sl.cold_total = cold_total;
    return CSR5HIP_SUCCESS;
}

// What a slab child has of its parent's options.  It takes ONLY the SpMV mode and the y-compaction and non-temporal requests;
// it never windows x, never builds slabs of its own and always walks XCD-contiguous ranges; every other request -- deferred
// carries, narrow and flagged columns among them -- keeps its default.  (The transposed companion, csr5_capi.hip
// inherit_companion, is the opposite: it copies everything but the snapshot.)
void inherit_child(csr5hip_handle c, const csr5hip_handle_s *h)
{
    c->req = Requests{};
    c->req.ldsy = h->req.ldsy;
    c->req.nt = h->req.nt;
    c->req.xwin = 0;
    c->req.slab = 0;
    c->opt.mode = h->opt.mode;
    c->opt.xcd_remap = 1;
}

// the stacked matrix: an ordinary CSR matrix with m2 rows, converted and multiplied by the ordinary kernels
int convert_child(SlabBuild &b)
{
    csr5hip_handle h = b.h;
    SlabStructure &sl = h->slab;
    const Geometry &g = h->g;
    hipStream_t s = h->stream;
    const bool hot = b.choice.verdict == SLAB_TABLE;
    csr5hip_handle c = sl.child ? sl.child : new csr5hip_handle_s(); // (kept across asCSR/asCSR5 cycles)
    sl.child = c;
    c->is_child = true;
    c->g.m = (int)b.m2;
    c->g.n = g.n;
    c->value_type = h->value_type;
    c->stream = s;
    inherit_child(c, h);
    c->hot_enabled = hot;
    c->d.col_lo = hot ? (const uint16_t *)sl[B_COL_LO].ptr : nullptr;
    c->d.col_hi = hot ? (const uint8_t *)sl[B_COL_HI].ptr : nullptr;
    c->d.slab_off = (const int32_t *)sl[B_SLAB_OFF].ptr;
    c->d.slab_shift = h->req.slab_shift;
    c->d.slab_bits = b.choice.bits;
    c->d.xperm = hot ? sl[B_XPERM].ptr : nullptr;
    c->d.cold_base = hot ? (const int32_t *)sl[B_COLD_BASE].ptr : nullptr;
    c->d.cold_cols = hot ? (const int32_t *)sl[B_COLD_COLS].ptr : nullptr;
    c->d.cold_total = hot ? sl.cold_total : 0;
    sl.xperm_valid = false;
    c->d.hot_cols = (const int32_t *)sl[B_HOT_COLS].ptr;
    c->d.hot_count = (const int32_t *)sl[B_HOT_COUNT].ptr;
    c->d.hot_tile0 = (const int32_t *)sl[B_HOT_TILE0].ptr;
    c->d.hot_slabs = b.choice.S;
    c->d.hot_capacity = b.plan.hot_capacity;
    c->d.range_lead = sl[B_LEAD].ptr;
    c->d.range_head = (uint32_t *)sl[B_RANGE_HEAD].ptr;
    c->d.range_begin = hot ? (const int32_t *)sl[B_RANGE_CUT].ptr : nullptr;
    int rc = csr5hip_input_csr(c, g.nnz, (int32_t *)sl[B_ROW_PTR2].ptr, (int32_t *)sl[B_COL2].ptr, sl[B_VAL2].ptr);
    c->sigma_request = hot ? b.plan.hot_sigma : g.sigma;
    if (rc == CSR5HIP_SUCCESS)
        rc = csr5hip_as_csr5(c);
    if (rc == CSR5HIP_SUCCESS && hot) {
        // which row every wavefront range of the persistent kernel starts in (k_range_finish adds the seams)
        hipError_t e = launch_range_heads(c->g, c->d, s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(s);
        if (e != hipSuccess)
            rc = fail_hip(e, "k_range_heads");
    }
    return rc;
}

// CSR5HIP_OPT_NARROW_VALUES at conversion: an error fails the build
int narrow_values(SlabBuild &b)
{
    csr5hip_handle h = b.h, c = h->slab.child;
    h->slab.values_narrowed = false;
    c->d.val32 = nullptr;
    if (!(b.choice.verdict == SLAB_TABLE && h->req.narrow && h->value_type == CSR5HIP_F64 && h->g.nnz > 0))
        return CSR5HIP_SUCCESS;
    bool narrow = false, copying = false;
    const hipError_t e = narrow_child_values(h, c, true, &narrow, &copying);
    if (e != hipSuccess)
        return fail_hip(e, "narrow values");
    if (narrow) {
        c->d.val32 = (const float *)h->slab[B_VAL32].ptr;
        h->slab.values_narrowed = true;
    }
    return CSR5HIP_SUCCESS;
}

// the phases in order; any failure is one return: build_slabs releases what was built
int build_slabs_impl(csr5hip_handle h)
{
    SlabStructure &sl = h->slab;
    sl.deactivate();
    sl.t_slab = 0;
    const double t0 = now_ms();
    SlabBuild b{};
    b.h = h;
    int rc = plan_slabs(h, &b.plan);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    if (!b.plan.S) {
        sl.release(); // not wanted (any more): give the memory back
        return CSR5HIP_SUCCESS;
    }
    rc = reserve_temporaries(b);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    struct TmpGuard { // very big temporaries (4 B per non-zero) do not outlive the build
        Buffer &b;
        size_t keep;
        ~TmpGuard()
        {
            if (b.cap > keep)
                b.release();
        }
    } tmp_guard{sl[B_TMP], b.tmp_keep};
    if (b.plan.hot) {
        rc = select_hot_columns(b);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
    }
    b.choice = slab_after_sample(b.plan, sl.hot_cover_pct);
    if (b.choice.verdict == SLAB_NONE) {
        // (nothing is active -- deactivate() above -- and the selection's buffers stay with the handle like every other
        //  buffer of the structure: freeing and re-allocating them was 0.3 of this path's 0.49 ms per reconversion of a
        //  3 M-nnz matrix; csr5hip_info.slab_hot_cover_pct keeps the estimate that explains the choice)
        sl.t_slab = now_ms() - t0; // (the column sample that decided it: part of the conversion's time)
        return CSR5HIP_SUCCESS;
    }
    rc = partition_segments(b);
    if (rc == CSR5HIP_SUCCESS && b.choice.verdict == SLAB_TABLE)
        rc = deal_and_pack(b);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream)); // (the temporaries are in use until here)
    rc = convert_child(b);
    if (rc == CSR5HIP_SUCCESS)
        rc = narrow_values(b);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    csr5hip_handle c = sl.child;
    if (c->hot_enabled) { // the range kernel this child launches needs the CU's whole LDS: raised here, once, not per SpMV
        const hipError_t e = prepare_spmv_hot(c->g, c->d, c->value_type, c->opt);
        if (e != hipSuccess)
            return fail_hip(e, "LDS limit of the range kernel");
    }
    sl.S = b.choice.S;
    sl.m2 = (int)b.m2;
    sl.sample_stride = b.plan.stride;
    sl.min_count = b.plan.min_count;
    sl.t_slab = now_ms() - t0;
    return CSR5HIP_SUCCESS;
}

} // namespace

namespace csr5 {

int build_slabs(csr5hip_handle h)
{
    h->slab.fallback = false;
    const int rc = build_slabs_impl(h);
    if (rc == CSR5HIP_SUCCESS) // (the plain path serves spmv() when no structure is active: its narrow column codes, if of use)
        return h->slab.S > 0 || h->is_child ? rc : prepare_plain(h);
    const std::string why = last_error();
    (void)hipGetLastError(); // clear a sticky allocation error
    h->slab.release();
    h->slab.fallback = true;
    h->drop_graphs();
    set_last_error("column slabs not built, plain tile kernel in use: " + why);
    if (h->req.slab >= 2)
        return rc;
    return prepare_plain(h);
}

// CSR5HIP_OPT_NARROW_VALUES: when every value is exactly representable in fp32 the range kernel streams them as fp32
// (converted back in registers: the same products, bit for bit); the fp64 array stays for the CSR tail and asCSR
hipError_t narrow_child_values(csr5hip_handle h, csr5hip_handle c, bool sync_copy, bool *narrow, bool *copying)
{
    *narrow = *copying = false;
    hipStream_t s = h->stream;
    const size_t nnz = (size_t)h->g.nnz;
    unsigned *flag = c->d.counters + 5;
    unsigned inexact = 1;
    hipError_t e = launch_fp32_exact((const double *)c->d.val, nnz, flag, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&inexact, flag, sizeof(inexact), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess || inexact)
        return e;
    *copying = true;
    e = h->slab[B_VAL32].reserve(nnz * sizeof(float));
    if (e == hipSuccess)
        e = launch_narrow((const double *)c->d.val, nnz, (float *)h->slab[B_VAL32].ptr, c->g.tile_elems, c->g.p - 1, s);
    if (e == hipSuccess && sync_copy)
        e = hipStreamSynchronize(s);
    *narrow = e == hipSuccess;
    return e;
}

} // namespace csr5
