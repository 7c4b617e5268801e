// csr5_convert.hip -- CSR -> CSR5 and back (csr5hip_as_csr5, csr5hip_as_csr): the pieces of the conversion, which csr5hip_load
// (csr5_checkpoint.hip) shares, the kernel-side tables of the plain path that are built on demand and the three rules that pick
// its kernel variant.  Host code only.
#include <cstring>
#include <string>

#include "csr5_handle.h"

using namespace csr5;

namespace csr5 {

// LDS x-window variant of the fused kernel: forced, or (auto) when the windows found at conversion
// cover at least XWIN_AUTO_COVER_PCT % of ALL non-zeros of the transposed tiles.  Measured on MI355X:
// ~95 % coverage (banded) -> 1.2-1.4x faster from 1.4 k to 28 k tiles; ~50 % coverage (half the
// columns random) -> 0-20 % slower, because every step still needs a divergent global gather.
int xwin_decision(const csr5hip_handle_s *h)
{
    constexpr int XWIN_AUTO_COVER_PCT = 70;
    constexpr int XWIN_AUTO_MIN_SIGMA = 16;
    constexpr int XWIN_AUTO_MIN_LINES_F64 = 16;
    if ((long long)h->g.n * (long long)h->vsize() >= (1LL << 31))
        return 0; // (the window kernel reads x through a buffer resource with 32-bit byte offsets)
    if (h->req.xwin == 2)
        return 1;
    if (h->req.xwin != 1 || h->g.p <= 1 || h->xwin_tiles <= 0)
        return 0;
    // Staging a 4-KB slice of x costs 8 (fp64) or 16 (fp32) coalesced wave loads, LDS writes and a wave barrier
    // per tile; it replaces sigma gather instructions.  Measured on MI355X (scripts/experiments/xwin_by_rowlen.py
    // and the bench stand-ins), the window pays only when
    //  (a) it covers most non-zeros,
    //  (b) sigma is large enough to amortise the staging (sigma = 6: 8-11 % SLOWER on scircuit-/webbase-like with
    //      80-95 % near-diagonal entries; sigma = 16: faster), and
    //  (c) for fp64, a gather instruction is spread over many 128-byte lines of x (nd24k-like: 25 lines, +9 %;
    //      columns within +-64 of the diagonal: 8 lines, -2 %); fp32 gains at any spread (nd24k-like 1.45x).
    const bool covered = (long long)h->xwin_covered * 100 >=
                         (long long)(h->g.p - 1) * h->g.tile_elems * XWIN_AUTO_COVER_PCT;
    const bool spread = h->value_type == CSR5HIP_F32 ||
                        h->xwin_lines >= (long long)XWIN_AUTO_MIN_LINES_F64 * h->xwin_tiles;
    return covered && h->g.sigma >= XWIN_AUTO_MIN_SIGMA && spread;
}

// y segments through LDS (coalesced flush): pays when a tile holds many rows.  Measured on MI355X
// (scripts/experiments/ldsy_by_rowlen.py): 5-15 % faster at 2-8 non-zeros per row, 1-3 % at 16, even at 20-32,
// 1-3 % slower beyond (one or two segments per tile: the compaction is pure overhead).
int ldsy_decision(const csr5hip_handle_s *h)
{
    if (h->req.ldsy == 2)
        return 1;
    if (h->req.ldsy != 1 || h->g.m <= 0)
        return 0;
    return (long long)h->g.nnz <= 20LL * h->g.m;
}

// Non-temporal stream loads: measured on MI355X +5 % on R-MAT 22 (0.8 GB of streams) and -18..25 % on matrices
// that fit the 256-MiB Infinity Cache (they are re-streamed from HBM by every SpMV instead of staying cached).
int nt_decision(const csr5hip_handle_s *h)
{
    if (h->req.nt == 2)
        return 1;
    if (h->req.nt != 1)
        return 0;
    const long long stream_bytes = (long long)h->g.nnz * (4 + (long long)h->vsize());
    return stream_bytes > 256LL * 1024 * 1024;
}

// ---- pieces of the conversion shared by csr5hip_as_csr5 and csr5hip_load -------------------------
// geometry from sigma (anonymouslib_cuda.h:121-137)
int derive_geometry(csr5hip_handle h, int sigma)
{
    Geometry &g = h->g;
    g.sigma = sigma;
    g.bit_y = bit_y_of(g.sigma);
    g.bit_all = g.bit_y + BIT_SS;
    if (g.bit_all > 31) // the first flag must sit in the first packet (anonymouslib_cuda.h:130)
        return CSR5HIP_UNSUPPORTED_CSR5_OMEGA;
    g.num_packet = num_packet_of(g.sigma);
    g.tile_elems = OMEGA * g.sigma;
    g.p = (int)(((long long)g.nnz + g.tile_elems - 1) / g.tile_elems);
    g.tail_start = g.m;
    g.defer = 0;
    h->num_offsets = 0;
    h->xwin_tiles = 0;
    h->xwin_covered = 0;
    h->xwin_lines = 0;
    h->opt.long_runs = 0;
    h->col16_built = false; // (the column words are about to be permuted again)
    h->col31_built = false;
    h->opt.col31 = 0;
    h->d.col31 = nullptr;
    h->opt.col16 = 0;
    h->d.col16 = nullptr;
    h->d.base16 = nullptr;
    h->t_malloc = h->t_tile_ptr = h->t_tile_desc = h->t_transpose = 0;
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

// the auxiliary arrays of the handle (anonymouslib_cuda.h:142-151) plus the carry state: one arena, its zero-initialised
// part cleared by ONE memset.  `offset` is sized by its upper bound (one slot per row start plus one per tile), so the
// conversion does not have to stop for the host to read num_offsets before it can continue (format_cuda.h:331-343
// does; that read now rides with the final one).
int reserve_aux(csr5hip_handle h)
{
    const Geometry &g = h->g;
    hipStream_t s = h->stream;
    const size_t p1 = (size_t)g.p + 1;
    // (a hot slab child keeps no descriptor array: see build_format_arrays)
    const size_t desc_words = h->is_child && h->hot_enabled ? OMEGA : (size_t)(g.p > 0 ? g.p : 1) * OMEGA * g.num_packet;
    const size_t offset_cap = h->is_child ? p1 : (size_t)g.m + p1; // (a slab child has no empty rows)
    h->scan_tmp_bytes = offset_scan_tmp_bytes((int)p1);
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    // zero-initialised part first
    const size_t o_desc = take(desc_words * 4), o_offp = take(p1 * 4), o_cal = take(p1 * h->vsize()),
                 o_acc = take(p1 * h->vsize()), o_cnt = take(p1 * 4), o_counters = take(COUNTER_WORDS * 4), o_tp = take(p1 * 4), o_offset = take(offset_cap * 4);
    const size_t zero_bytes = off;
    const size_t o_meta = take(p1 * 16), o_hdr = take(p1 * 32), o_scan = take(h->scan_tmp_bytes);
    HIP_TRY(h->b_arena.reserve(off));
    char *base = (char *)h->b_arena.ptr;
    h->d.tile_desc = (uint32_t *)(base + o_desc);
    h->d.offset_ptr = (int32_t *)(base + o_offp);
    h->d.calibrator = base + o_cal;
    h->d.carry_acc = base + o_acc;
    h->d.carry_cnt = (uint32_t *)(base + o_cnt);
    h->d.counters = (uint32_t *)(base + o_counters);
    h->d.offset = (int32_t *)(base + o_offset);
    h->d.tile_ptr = (uint32_t *)(base + o_tp);
    h->d.carry_meta = (uint32_t *)(base + o_meta);
    h->d.tile_hdr = (uint32_t *)(base + o_hdr);
    h->scan_tmp = base + o_scan;
    HIP_TRY(hipMemsetAsync(base, 0, zero_bytes, s));
    return CSR5HIP_SUCCESS; // stream-ordered: the conversion kernels follow on the same stream
}

// the two words the host needs from the conversion -- tail start and number of offsets, as in the reference
// (anonymouslib_cuda.h:165-167, format_cuda.h:331-343) -- copied asynchronously; valid after the next synchronisation
hipError_t read_format_scalars(csr5hip_handle h, bool sync)
{
    const Geometry &g = h->g;
    h->scalar_words[0] = h->scalar_words[1] = 0;
    if (g.p <= 0)
        return hipSuccess;
    hipError_t e = hipMemcpyAsync(&h->scalar_words[0], h->d.tile_ptr + (g.p - 1), 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&h->scalar_words[1], h->d.offset_ptr + g.p, 4, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && sync)
        e = hipStreamSynchronize(h->stream);
    return e;
}
void finish_format_scalars(csr5hip_handle h)
{
    if (h->g.p <= 0)
        return;
    h->g.tail_start = (int)(h->scalar_words[0] & ROW_MASK);
    h->num_offsets = (int)h->scalar_words[1];
}

// ---- narrow column codes (csr5_format.hip k_col16, csr5_spmv.hip C16) ---------------------------------------------------
// Only the x-window kernel reads them (a matrix whose tiles are covered by 4-KB windows of x has local columns), so they are
// built when that kernel is selected: one pass over the tile-ordered column words + one synchronisation for the count of wide
// tiles; 2 bytes per non-zero of device memory.  Stays valid until the next conversion.
int prepare_col16(csr5hip_handle h)
{
    h->opt.col16 = 0;
    h->d.col16 = nullptr;
    h->d.base16 = nullptr;
    const Geometry &g = h->g;
    const bool windowed = h->opt.x_window != 0;
    if (h->req.col16 == 0 || h->is_child || g.p <= 1 || h->opt.mode != 1 || !windowed || !col16_sigma(g.sigma))
        return CSR5HIP_SUCCESS;
    const size_t code_words = (size_t)(g.p - 1) * (g.tile_elems / 2);
    if (!h->col16_built) {
        // The codes are an optional accelerator (2 bytes per non-zero of device memory): when they cannot be built the handle
        // stays on the 32-bit column words -- csr5hip_last_error() says so -- instead of failing asCSR5() / setOption().
        uint32_t *wide = h->d.counters + 5;
        hipError_t e = h->b_col16.reserve((code_words + (size_t)g.p + 1) * 4);
        if (e == hipSuccess)
            e = hipMemsetAsync(wide, 0, 4, h->stream);
        if (e == hipSuccess)
            e = launch_col16(g, h->d, (uint32_t *)h->b_col16.ptr, (int32_t *)h->b_col16.ptr + code_words, wide, h->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(&h->col16_wide, wide, 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError(); // clear the sticky allocation / launch error
            h->b_col16.release();
            set_last_error(std::string("narrow column codes not built, 32-bit column words in use: ") + hipGetErrorString(e));
            h->drop_graphs();
            return CSR5HIP_SUCCESS;
        }
        h->col16_built = true;
    }
    if (h->col16_wide == 0) {
        h->d.col16 = (const uint32_t *)h->b_col16.ptr;
        h->d.base16 = (const int32_t *)h->b_col16.ptr + code_words;
        h->opt.col16 = 1;
    }
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

// ---- flagged column words (csr5_format.hip k_col31, csr5_spmv.hip C31) ----------------------------------------------------
// The plain fused kernel at sigma 4..8 (short rows: the auto rule's r = 6 / 8) reads its column words from a kernel-side copy
// that carries the element's row-start flag in bit 31: no descriptor load (256 B of a sigma = 6 tile's 4.9 KB and one of its
// load instructions), y_offset recomputed from the flags by a wave prefix sum as in the narrow-codes kernel; same gathers, same
// arithmetic, bit-identical results.  An optional accelerator (+4 bytes per non-zero of device memory): when it cannot be built
// the handle stays on column_index + tile_desc.  Not for the x-window kernel (it has the narrow codes) nor for a slab child.
// Auto rule (same-call A/B, scripts/experiments/round6/flagged_ab.py, profiles/r06_probes.txt section 4): the descriptor load rides
// in the tile's first round trip, so dropping it saves BYTES, not latency, and the flag extraction + prefix sum run after the data
// has arrived -- a matrix that streams from HBM gains (2 M rows x 27 per row, sigma 8: 168.9 -> 165.2 us, -2.2 %), the latency-bound
// stand-ins lose (scircuit-like +0.7 % cold, webbase-like without slabs +1.1 %, their local variants +3..5 %): on only when the
// streams exceed the Infinity Cache (the non-temporal rule's size).
int prepare_col31(csr5hip_handle h)
{
    h->opt.col31 = 0;
    h->d.col31 = nullptr;
    const Geometry &g = h->g;
    const bool pays = (long long)g.nnz * (4 + (long long)h->vsize()) > 256LL * 1024 * 1024;
    if (h->req.col31 == 0 || (h->req.col31 == 1 && !pays) || h->is_child || g.p <= 1 || h->opt.mode != 1 || h->opt.x_window ||
        !col31_sigma(g.sigma)) {
        h->drop_graphs();
        return CSR5HIP_SUCCESS;
    }
    if (!h->col31_built) {
        hipError_t e = h->b_col31.reserve((size_t)(g.p - 1) * g.tile_elems * 4);
        if (e == hipSuccess)
            e = launch_col31(g, h->d, (uint32_t *)h->b_col31.ptr, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError(); // clear the sticky allocation / launch error
            h->b_col31.release();
            set_last_error(std::string("flagged column words not built, column_index + tile_desc in use: ") + hipGetErrorString(e));
            h->drop_graphs();
            return CSR5HIP_SUCCESS;
        }
        h->col31_built = true;
    }
    h->d.col31 = (const uint32_t *)h->b_col31.ptr;
    h->opt.col31 = 1;
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

// kernel-side tables of the plain (non-slab) path that are built on demand: the narrow column codes of the x-window kernel,
// else the flagged column words of the plain kernel
int prepare_plain(csr5hip_handle h)
{
    const int rc = prepare_col16(h);
    return rc != CSR5HIP_SUCCESS ? rc : prepare_col31(h);
}

// what the fused kernel needs on top of the reference's format arrays: carry meta, x windows, tile headers
int derive_kernel_tables(csr5hip_handle h)
{
    // Deferred carries (CSR5HIP_OPT_DEFER_CARRIES), decided BEFORE the carry meta is written: forced, or (auto) a fused-mode matrix
    // of many tiles.  There the cut rows cost the one-tile kernel twice: a returning atomic at the end of a tile for every
    // hand-shake, and -- for the short-spill ownership that avoids most hand-shakes -- two scattered loads and a gather of the
    // NEXT tile's first 64 elements in every tile (sigma cache lines each: + 2/3 of a sigma = 24 fp32 tile's own lines).  With
    // the flag set no tile finishes its neighbour's spill, every meeting of partials is parked with plain stores and
    // k_calibrate (one thread per tile, ~3 us) adds them: nd24k-like fp32 cold 50.5 -> 37.5 us.  Small matrices keep the
    // in-launch protocol: a second launch costs them more than it saves (rule: csr5_internal.h DEFER_AUTO_*).
    {
        const Geometry &g0 = h->g;
        const bool long_rows = (long long)g0.nnz >= (long long)DEFER_AUTO_LONG_ROW * (g0.m > 0 ? g0.m : 1);
        const bool pays = long_rows ? g0.p - 1 >= DEFER_AUTO_MIN_TILES_LONG
                                    : (long long)(g0.p - 1) * g0.sigma >= DEFER_AUTO_MIN_TILE_SIGMA;
        h->g.defer = !h->is_child && h->opt.mode == 1 && g0.p > 1 && (h->req.defer == 2 || (h->req.defer == 1 && pays)) ? 1 : 0;
    }
    const Geometry &g = h->g;
    hipStream_t s = h->stream;
    if (!h->host_words) {
        HIP_TRY(hipHostMalloc((void **)&h->host_words, 128, hipHostMallocDefault));
        memset(h->host_words, 0, 128);
        int dev = 0, khz = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
            h->wall_clock_khz = khz;
        else
            h->wall_clock_khz = 100000.0; // gfx9: 100 MHz
    }
    // carry_meta + x-windows + fused-kernel headers in one launch, then the export of the host's words
    HIP_TRY(launch_tile_tables(g, h->d, (int)h->vsize(), h->host_words, h->is_child && h->hot_enabled, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t *w = h->host_words;
    h->scalar_words[0] = w[0];
    h->scalar_words[1] = w[1];
    finish_format_scalars(h);
    h->xwin_tiles = (int)w[2];
    h->xwin_covered = (long long)w[3];
    h->opt.long_runs = w[4] != 0;
    h->xwin_lines = (long long)w[5];
    if (g.defer)
        h->opt.long_runs = 1; // (the parties of every cut row park: k_calibrate is part of each SpMV)
    // phase times from the kernels' wall-clock stamps (k_row_scan, k_tile_desc, k_transpose, k_tile_tables); a phase
    // whose kernel did not run (single-tile matrices) has no stamp and takes the next one's
    unsigned long long st[4];
    memcpy(st, w + 8, sizeof(st));
    for (int i = 2; i >= 0; i--)
        if (!st[i])
            st[i] = st[i + 1];
    const double per_tick_ms = 1.0 / h->wall_clock_khz;
    h->t_tile_ptr += (double)(st[1] - st[0]) * per_tick_ms;
    h->t_tile_desc += (double)(st[2] - st[1]) * per_tick_ms;
    h->t_transpose += (double)(st[3] - st[2]) * per_tick_ms;
    return CSR5HIP_SUCCESS;
}

// steps 1-2 of the conversion: everything that is derived from row_ptr alone (tile_ptr, tile_desc, offset_ptr,
// offset).  Stream-ordered, no host round trip (see reserve_aux).
int build_format_arrays(csr5hip_handle h)
{
    Geometry &g = h->g;
    hipStream_t s = h->stream;
    // step 1: tile_ptr (+ empty-row marks) -- flag scatter shares the row pass
    HIP_TRY(launch_row_scan(g, h->d, s));
    // A hot slab child needs nothing else: its bit flags ride in the packed column codes, the range kernel recomputes
    // y_offset from them, and it has no empty rows (no offsets).  (k_tile_desc on the 40 M-row child of R-MAT 24: 0.4 ms.)
    if (h->is_child && h->hot_enabled)
        return CSR5HIP_SUCCESS;

    // step 2: tile_desc, offset_ptr scan, empty-row offsets (the kernel leaves unflagged tiles at once)
    HIP_TRY(launch_tile_desc(g, h->d, s));
    HIP_TRY(launch_offset_scan(g, h->d, h->scan_tmp, h->scan_tmp_bytes, s));
    HIP_TRY(launch_desc_offset(g, h->d, s));
    return CSR5HIP_SUCCESS;
}

void resolve_variants(csr5hip_handle h)
{
    h->opt.x_window = xwin_decision(h);
    h->opt.lds_y = ldsy_decision(h);
    h->opt.stream_nt = nt_decision(h);
    h->opt.hot = h->hot_enabled ? 1 : 0;
}

} // namespace csr5

extern "C" {

int csr5hip_as_csr5(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_SUCCESS;
    if (h->format != CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNKOWN_FORMAT;
    if (h->sigma_request < CSR5HIP_MIN_SIGMA)
        h->sigma_request = csr5hip_auto_sigma(h->g.m, h->g.nnz, h->value_type);

    int rc = derive_geometry(h, h->sigma_request);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    Geometry &g = h->g;
    hipStream_t s = h->stream;

    // ONE host round trip in all, at the end (the reference synchronises after every phase and reads two words in
    // between, anonymouslib_cuda.h:161-208).  The four phase times the reference prints are taken from wall-clock stamps of
    // the stream instead of host timers around synchronisations.
    double t0 = now_ms();
    rc = reserve_aux(h);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    h->t_malloc += now_ms() - t0;

    if (g.p > 0) {
        rc = build_format_arrays(h);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
        // step 3: in-place tile transpose of column_index and value, then the kernel-side tables
        if (h->is_child && h->hot_enabled)
            HIP_TRY(launch_transpose_values(g, h->d, h->value_type, s)); // (the column codes are read in CSR order)
        else
            HIP_TRY(launch_transpose(g, h->d, h->value_type, true, s));
        // From here on the caller's arrays are in tile order while the handle still says CSR: a failure must
        // put them back (a retry would transpose them a second time).
        auto finish = [&]() -> int {
            return derive_kernel_tables(h); // ends with the one synchronisation; phase times from the kernels' stamps
        };
        rc = finish();
        if (rc != CSR5HIP_SUCCESS) {
            const std::string why = last_error();
            if (h->is_child && h->hot_enabled)
                h->format = -1; // only the VALUES of every tile were transposed (private arrays of a slab structure, which the
                                // parent releases on failure): nothing to restore, the handle is unusable until inputCSR
            else if (launch_transpose(g, h->d, h->value_type, false, s) != hipSuccess ||
                     hipStreamSynchronize(s) != hipSuccess)
                h->format = -1; // the arrays could not be restored: the handle is unusable until inputCSR
            set_last_error(why);
            return rc;
        }
    } else {
        HIP_TRY(hipStreamSynchronize(s));
    }
    resolve_variants(h);
    h->format = CSR5HIP_FORMAT_CSR5;
    rc = build_slabs(h); // (ends with prepare_plain when the plain path serves spmv())
    if (rc != CSR5HIP_SUCCESS) {
        // only when the structure was requested explicitly: a failed asCSR5 leaves CSR, as in the reference
        // (anonymouslib_cuda.h:105-220 returns before _format changes)
        const std::string why = last_error();
        if (csr5hip_as_csr(h) != CSR5HIP_SUCCESS)
            h->format = -1; // the arrays could not be restored: unusable until inputCSR
        set_last_error(why);
    }
    return rc;
}

int csr5hip_as_csr(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_SUCCESS;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    h->drop_graphs();
    h->slab.deactivate();
    HIP_TRY(launch_transpose(h->g, h->d, h->value_type, false, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->b_spmm.release(); // (the SpMM workspace is sized by the converted matrix: released with it)
    h->comp.release(); // (so is the transposed companion)
    // the aux buffers stay cached in the handle (capacity only grows) until csr5hip_free
    h->format = CSR5HIP_FORMAT_CSR;
    return CSR5HIP_SUCCESS;
}

int csr5hip_destroy(csr5hip_handle h) { return csr5hip_as_csr(h); }

} // extern "C"
