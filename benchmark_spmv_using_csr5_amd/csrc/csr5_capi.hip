// csr5_capi.hip -- the extern "C" boundary of libcsr5hip.so (declared in include/csr5hip.h).
//
// State machine and ownership follow the reference handle (CSR5_cuda/anonymouslib_cuda.h):
//   inputCSR borrows the caller's device CSR arrays and sets _format = CSR          (:61-76)
//   asCSR5   builds tile_ptr / tile_desc / offsets and transposes col/val IN PLACE  (:105-220)
//   spmv     returns UNSUPPORTED_CSR_SPMV (-4) while the format is CSR              (:262-284)
//   asCSR / destroy undo the transpose and drop the CSR5 arrays                     (:78-102, :286-291)
//
// This unit: create / free, options, setX, the entry points, graphs, info and the device shims.  The conversion lives in
// csr5_convert.hip, the checkpoint in csr5_checkpoint.hip, the column-slab build in csr5_slab_build.hip; csr5_handle.h has the handle.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csr5_handle.h"

using namespace csr5;

namespace {

thread_local std::string g_last_error;

} // namespace

namespace csr5 {
void set_last_error(const std::string &msg) { g_last_error = msg; }
const std::string &last_error() { return g_last_error; }

int fail_hip(hipError_t e, const char *what)
{
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
    return CSR5HIP_HIP_ERROR;
}

// the transposed companion and everything held for it (csr5hip_build_transpose)
void Companion::release()
{
    if (at) {
        csr5hip_free(at);
        at = nullptr;
    }
    built = false;
    t_build = 0;
    for (Buffer &b : buf)
        b.release();
}

long long Companion::bytes() const
{
    long long sum = 0;
    for (const Buffer &b : buf)
        sum += (long long)b.cap;
    return sum;
}
} // namespace csr5

extern "C" {

const char *csr5hip_last_error(void) { return g_last_error.c_str(); }
const char *csr5hip_version(void) { return "csr5hip 0.1 (gfx950, omega=64)"; }

int csr5hip_create(csr5hip_handle *out, int m, int n, int value_type)
{
    if (!out || m < 0 || n < 0)
        return CSR5HIP_INVALID_ARGUMENT;
    if (value_type != CSR5HIP_F64 && value_type != CSR5HIP_F32)
        return CSR5HIP_UNSUPPORTED_VALUE_TYPE;
    csr5hip_handle h = new csr5hip_handle_s();
    h->g.m = m;
    h->g.n = n;
    h->value_type = value_type;
    *out = h;
    return CSR5HIP_SUCCESS;
}

int csr5hip_free(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    h->drop_graphs();
    h->comp.release();
    h->slab.release();
    h->b_arena.release();
    h->b_col16.release();
    h->b_col31.release();
    h->b_spmm.release();
    if (h->host_words)
        (void)hipHostFree(h->host_words);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
    return CSR5HIP_SUCCESS;
}

int csr5hip_set_stream(csr5hip_handle h, void *hip_stream)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    h->stream = (hipStream_t)hip_stream;
    h->slab.xperm_valid = false; // (snapshot mode: the copy was taken on the old stream; the new one takes its own, in order)
    h->drop_graphs();
    if (h->comp.at) // (the companion lives on its parent's stream)
        return csr5hip_set_stream(h->comp.at, hip_stream);
    return CSR5HIP_SUCCESS;
}

int csr5hip_warmup(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    HIP_TRY(launch_warmup(h->stream));
    return CSR5HIP_SUCCESS;
}

int csr5hip_input_csr(csr5hip_handle h, int nnz, int32_t *d_row_ptr, int32_t *d_col_idx, void *d_val)
{
    if (!h || nnz < 0)
        return CSR5HIP_INVALID_ARGUMENT;
    h->comp.release(); // (it belonged to the matrix that is being replaced)
    h->format = CSR5HIP_FORMAT_CSR;
    h->g.nnz = nnz;
    h->d.row_ptr = d_row_ptr;
    h->d.col = d_col_idx;
    h->d.val = d_val;
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

int csr5hip_set_x(csr5hip_handle h, const void *d_x)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    h->x = d_x;
    h->slab.xperm_valid = false; // (snapshot mode: the next spmv() takes a new copy)
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

// gfx950 tables in the shape of the reference's (r, s, t, u) rule (anonymouslib_cuda.h:297-313, one table per
// architecture and precision there too): k = nnz/m; sigma = r if k <= r; k if k <= s; s if k <= t; else u.
// fp64: (6, 16, 256, 16); fp32: (8, 16, 256, 16) -- from sweeps of all sigma over mean row lengths 2..512, random and
// near-diagonal columns (scripts/experiments/sigma_table.py; profiles/r01_sigma_table.txt, re-run on the round-4 kernels in
// profiles/r04_sigma_table.txt): the sigma surface is flat on gfx950 and the rules stay within a few per cent of the measured
// best everywhere.  r = 6 instead of the reference's 4 costs random-column fp64 matrices < 1 % and gains 4-8 % where the
// columns are local; fp32 rows are half as wide, so a tile of the same byte size holds twice the elements: short rows
// (k <= 8) with local columns ran 5-8 % faster at sigma = 8 than at 6, at no cost with random columns.  Beyond 256
// non-zeros per row sigma = 32 would gain 3-7 % on random columns but loses 10 % on the nd24k-like stand-in (x-window +
// jitter): u = 16 for fp64.  fp32: 24 won by 3 % for a while in round 5 (a 6-KB tile like fp64's sigma = 16); since the narrow
// codes carry the row-start flags the sigma = 24 kernel needs 136 VGPRs (3 wavefronts per SIMD) and sigma = 16 (78 VGPRs, 6 per
// SIMD) wins: nd24k-like 29.1 / 37.0 us warm / cold against 31.7 / 38.9: u = 16 again.
int csr5hip_auto_sigma(int m, int nnz, int value_type)
{
    const int r = value_type == CSR5HIP_F32 ? 8 : 6, s = 16, t = 256, u = 16;
    const int k = m > 0 ? nnz / m : 0;
    if (k <= r) return r;
    if (k <= s) return k;
    if (k <= t) return s;
    return u;
}

int csr5hip_set_sigma(csr5hip_handle h, int sigma)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    const bool is_auto = sigma == CSR5HIP_AUTO_TUNED_SIGMA;
    if (is_auto)
        sigma = csr5hip_auto_sigma(h->g.m, h->g.nnz, h->value_type);
    if (sigma < CSR5HIP_MIN_SIGMA || sigma > CSR5HIP_MAX_SIGMA)
        return CSR5HIP_INVALID_ARGUMENT;
    h->sigma_request = sigma;
    h->sigma_auto = is_auto;
    return CSR5HIP_SUCCESS;
}

static int set_option_impl(csr5hip_handle h, int option, int value);

// A transposed companion carries every option of its parent except CSR5HIP_OPT_X_SNAPSHOT (spmv_t takes x per call and reads it live)
int csr5hip_set_option(csr5hip_handle h, int option, int value)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    const int rc = set_option_impl(h, option, value);
    if (rc != CSR5HIP_SUCCESS || !h->comp.at || option == CSR5HIP_OPT_X_SNAPSHOT)
        return rc;
    return set_option_impl(h->comp.at, option, value);
}

static int set_option_impl(csr5hip_handle h, int option, int value)
{
    switch (option) {
    case CSR5HIP_OPT_SPMV_MODE:
        if (value != 0 && value != 1)
            return CSR5HIP_INVALID_ARGUMENT;
        h->opt.mode = value;
        if (h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0) {
            const int rc = prepare_plain(h);
            if (rc != CSR5HIP_SUCCESS)
                return rc;
        }
        if (h->slab.S > 0 && h->slab.child->hot_enabled && value != 1) {
            // the hot table exists for the fused kernel only and its column words are encoded: rebuild without it
            h->drop_graphs();
            return build_slabs(h);
        }
        break;
    case CSR5HIP_OPT_XCD_REMAP:
        h->opt.xcd_remap = value ? 1 : 0;
        break;
    case CSR5HIP_OPT_LDS_Y:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.ldsy = value;
        if (h->format == CSR5HIP_FORMAT_CSR5)
            h->opt.lds_y = ldsy_decision(h);
        break;
    case CSR5HIP_OPT_STREAM_NT:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.nt = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->opt.stream_nt = nt_decision(h);
            if (h->is_child && h->hot_enabled) // another instantiation of the range kernel: its LDS limit
                HIP_TRY(prepare_spmv_hot(h->g, h->d, h->value_type, h->opt));
        }
        break;
    case CSR5HIP_OPT_X_WINDOW:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.xwin = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->opt.x_window = xwin_decision(h);
            const int rc = h->slab.S <= 0 ? prepare_plain(h) : CSR5HIP_SUCCESS;
            if (rc != CSR5HIP_SUCCESS)
                return rc;
        }
        break;
    case CSR5HIP_OPT_COLUMN_SLABS:
        if (value < 0 || value > 64 || (value & (value - 1)))
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.slab = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->drop_graphs();
            return build_slabs(h);
        }
        break;
    case CSR5HIP_OPT_SLAB_SHIFT:
        if (value < 0 || value > 24)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.slab_shift = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->drop_graphs();
            return build_slabs(h);
        }
        break;
    case CSR5HIP_OPT_SLAB_HOT:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.hot = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->drop_graphs();
            return build_slabs(h);
        }
        break;
    case CSR5HIP_OPT_ZERO_EMPTY_ROWS:
        h->req.zero_empty = value ? 1 : 0;
        break;
    case CSR5HIP_OPT_X_SNAPSHOT:
        if (value != 0 && value != 1)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.x_snapshot = value;
        h->slab.xperm_valid = false;
        break;
    case CSR5HIP_OPT_NARROW_VALUES:
        if (value != 0 && value != 1)
            return CSR5HIP_INVALID_ARGUMENT;
        if (h->req.narrow != value) {
            h->req.narrow = value;
            if (h->format == CSR5HIP_FORMAT_CSR5) {
                h->drop_graphs();
                return build_slabs(h);
            }
        }
        break;
    case CSR5HIP_OPT_DEFER_CARRIES:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        if (h->format == CSR5HIP_FORMAT_CSR5 && value != h->req.defer) {
            set_last_error("CSR5HIP_OPT_DEFER_CARRIES takes effect at asCSR5(): set it while the matrix is in CSR form");
            return CSR5HIP_INVALID_ARGUMENT;
        }
        h->req.defer = value;
        break;
    case CSR5HIP_OPT_NARROW_COLUMNS:
        if (value != 0 && value != 1)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.col16 = value;
        if (h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0) {
            const int rc = prepare_col16(h);
            if (rc != CSR5HIP_SUCCESS)
                return rc;
        }
        break;
    case CSR5HIP_OPT_FLAGGED_COLUMNS:
        if (value < 0 || value > 2)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.col31 = value;
        if (h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0) {
            const int rc = prepare_col31(h);
            if (rc != CSR5HIP_SUCCESS)
                return rc;
        }
        break;
    case CSR5HIP_OPT_SLAB_MEMORY_MIB:
        if (value < 0)
            return CSR5HIP_INVALID_ARGUMENT;
        h->req.slab_mem_mib = value;
        if (h->format == CSR5HIP_FORMAT_CSR5) {
            h->drop_graphs();
            return build_slabs(h);
        }
        break;
    default:
        return CSR5HIP_INVALID_ARGUMENT;
    }
    if (h->slab.S > 0 && (option == CSR5HIP_OPT_SPMV_MODE || option == CSR5HIP_OPT_LDS_Y || option == CSR5HIP_OPT_STREAM_NT))
        csr5hip_set_option(h->slab.child, option, value);
    h->drop_graphs();
    return CSR5HIP_SUCCESS;
}

static bool stream_is_capturing(hipStream_t s)
{
    if (s == nullptr)
        return false;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError(); // (the query itself failed: treat the stream as not capturing)
        return false;
    }
    return cap != hipStreamCaptureStatusNone;
}

// CSR5HIP_OPT_X_SNAPSHOT: the permuted copy of x is taken once per setX -- here, on stream s, in front of the first SpMV
// (or graph capture) that needs it
static hipError_t ensure_x_snapshot(csr5hip_handle h, hipStream_t s)
{
    if (!h->req.x_snapshot || h->slab.xperm_valid || h->slab.S <= 0 || !h->slab.child->hot_enabled)
        return hipSuccess;
    // a caller capturing its own graph gets the copy recorded with every spmv() (enqueue_spmv)
    if (stream_is_capturing(s))
        return hipSuccess;
    hipError_t e = launch_x_permute(h->slab.child->g, h->slab.child->d, h->value_type, h->x, s);
    if (e == hipSuccess)
        h->slab.xperm_valid = true;
    return e;
}

// one SpMV on stream s: the tile kernel on the matrix itself, or -- with column slabs -- on the stacked matrix
// followed by the combine kernel.  own_graph: s is the private capture stream of spmv_repeat / spmv_rotate, whose graphs
// set_x drops; otherwise s is the caller's stream, which may itself be capturing.
static hipError_t enqueue_spmv(csr5hip_handle h, void *d_y, hipStream_t s, bool own_graph)
{
    if (h->slab.S > 0) {
        csr5hip_handle c = h->slab.child;
        hipError_t e = hipSuccess;
        // CSR5HIP_OPT_X_SNAPSHOT: the copy taken at the last setX may be reused -- except inside a graph the CALLER is
        // capturing: that graph outlives this setX (the handle cannot drop it), so it must carry the copy itself; a replay
        // after the caller rewrote x and called setX again would otherwise read the old copy
        const bool reuse = h->req.x_snapshot && h->slab.xperm_valid && (own_graph || !stream_is_capturing(s));
        if (c->hot_enabled && !reuse) {
            // the packed codes index the permuted copy of x: taken by every spmv() (x is read live, as the reference reads
            // it), or -- CSR5HIP_OPT_X_SNAPSHOT -- once per setX
            e = launch_x_permute(c->g, c->d, c->value_type, h->x, s);
            if (e != hipSuccess)
                return e;
        }
        e = launch_spmv(c->g, c->d, c->value_type, h->x, h->slab[B_P].ptr, c->opt, s);
        if (e != hipSuccess)
            return e;
        return launch_slab_combine(h->g.m, h->g.tail_start, h->req.zero_empty, h->slab.S, h->value_type,
                                   (const uint32_t *)h->slab[B_BASE].ptr, (const unsigned char *)h->slab[B_ROWIDX].ptr,
                                   (const uint32_t *)h->slab[B_NONEMPTY].ptr, h->slab[B_P].ptr, h->slab.m2, d_y, s);
    }
    if (h->req.zero_empty && h->g.m > 0) {
        // every row that owns a non-zero is overwritten by the kernel; this defines the others
        hipError_t e = hipMemsetAsync(d_y, 0, (size_t)h->g.m * h->vsize(), s);
        if (e != hipSuccess)
            return e;
    }
    return launch_spmv(h->g, h->d, h->value_type, h->x, d_y, h->opt, s);
}

int csr5hip_spmv(csr5hip_handle h, double alpha, void *d_y)
{
    (void)alpha; // accepted, not applied: csr5_spmv_cuda.h:22 ("// * alpha")
    if (!h || !d_y)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (!h->x)
        return CSR5HIP_INVALID_ARGUMENT;
    HIP_TRY(ensure_x_snapshot(h, h->stream));
    HIP_TRY(enqueue_spmv(h, d_y, h->stream, false));
    return CSR5HIP_SUCCESS;
}

// Y = A * X for k dense vectors (csr5_spmm.hip).  Runs on the handle's own tile structure whatever path spmv() takes (column
// slabs, hot table, x-window, fused mode ...): per column bit-identical to the two-pass spmv().  Reads neither the handle's x
// nor its snapshot.  The carry workspace is allocated by the first call that needs it; later calls only enqueue.
int csr5hip_spmm(csr5hip_handle h, const void *d_X, int ldx, int k, void *d_Y, int ldy)
{
    if (!h || k < 0 || ldx < k || ldy < k || (k > 0 && (!d_X || !d_Y)))
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (k == 0)
        return CSR5HIP_SUCCESS;
    const size_t work = (size_t)(h->g.p > 0 ? h->g.p : 1) * spmm_block_width(k) * h->vsize();
    if (h->b_spmm.cap < work) {
        const hipError_t e = h->b_spmm.reserve(work);
        if (e != hipSuccess) {
            (void)hipGetLastError(); // (clear the sticky allocation error: the handle stays usable for spmv)
            return fail_hip(e, "csr5hip_spmm: workspace");
        }
    }
    HIP_TRY(launch_spmm(h->g, h->d, h->value_type, d_X, ldx, k, d_Y, ldy, h->b_spmm.ptr, h->req.zero_empty, h->opt.xcd_remap, h->stream));
    return CSR5HIP_SUCCESS;
}

// out[e] = dot(U[row(e), :], V[col(e), :]) for every stored element, CSR order (csr5_sddmm.hip).  Runs on the handle's own tile
// structure whatever path spmv() takes; reads only pattern-derived arrays; allocates nothing: enqueue-only from the first call.
int csr5hip_sddmm(csr5hip_handle h, const void *d_U, int ldu, const void *d_V, int ldv, int k, void *d_out_csr)
{
    if (!h || k < 0 || ldu < k || ldv < k)
        return CSR5HIP_INVALID_ARGUMENT;
    const int nnz = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5 ? h->g.nnz : 0;
    if (nnz > 0 && ((k > 0 && (!d_U || !d_V)) || !d_out_csr))
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (nnz == 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_sddmm(h->g, h->d, h->value_type, d_U, ldu, d_V, ldv, k, d_out_csr, h->stream));
    return CSR5HIP_SUCCESS;
}

// Y[i, c] = max / min over row i's entries of a_e X[col(e), c] with its argmax (csr5_reduce.hip; the contract: csr5hip_reduce.h).
// Runs on the handle's own tile structure whatever path spmv() takes; reads the pattern and, weighted, the tile-ordered values;
// allocates nothing: enqueue-only from the first call.
int csr5hip_spmm_reduce(csr5hip_handle h, int op, int weighted, const void *d_X, int ldx, int k, void *d_Y, int ldy, int32_t *d_arg,
                        int ldarg)
{
    if (!h || (op != CSR5HIP_REDUCE_MAX && op != CSR5HIP_REDUCE_MIN) || (weighted != 0 && weighted != 1) || k < 0 || ldx < k ||
        ldy < k || (d_arg && ldarg < k) || (k > 0 && h->g.m > 0 && (!d_X || !d_Y)))
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (k == 0 || h->g.m <= 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_spmm_reduce(h->g, h->d, h->value_type, op, weighted, d_X, ldx, k, d_Y, ldy, d_arg, ldarg, h->stream));
    return CSR5HIP_SUCCESS;
}

// Its gradients in up to two launches: dval by a row kernel on the parent's pattern, dX by a column kernel on the transposed
// companion's (its source map, comp[A_MAP], passed, not copied; weighted: its copy of the values).  A launch whose output is null is
// not made.  Allocates nothing, changes nothing of the handle or of its companion: enqueue-only.
int csr5hip_spmm_reduce_backward(csr5hip_handle h, int weighted, const void *d_X, int ldx, int k, const void *d_dY, int lddy,
                                 const int32_t *d_arg, int ldarg, void *d_dX, int lddx, void *d_dval_csr)
{
    if (!h || (weighted != 0 && weighted != 1) || k < 0 || ldx < k || lddy < k || ldarg < k || lddx < k || (d_dval_csr && !weighted))
        return CSR5HIP_INVALID_ARGUMENT;
    if (k > 0 && h->g.m > 0 && ((d_dval_csr && !d_X) || !d_dY || !d_arg))
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (d_dX && !h->comp.built) {
        g_last_error = "csr5hip_spmm_reduce_backward: dX needs the transposed companion, call csr5hip_build_transpose first";
        return CSR5HIP_INVALID_ARGUMENT;
    }
    if (d_dval_csr && h->g.nnz > 0) {
        if (k > 0 && h->g.m > 0)
            HIP_TRY(launch_spmm_reduce_dval(h->g, h->d, h->value_type, d_X, ldx, k, d_dY, lddy, d_arg, ldarg, d_dval_csr, h->stream));
        else // (no column to win in: every entry's chain is empty)
            HIP_TRY(hipMemsetAsync(d_dval_csr, 0, (size_t)h->g.nnz * h->vsize(), h->stream));
    }
    if (d_dX && k > 0 && h->g.n > 0) {
        if (h->g.nnz == 0 || h->g.m <= 0 || !h->comp.at || !h->comp[A_MAP].ptr) // no entries (and then no companion arrays): the zeros
            HIP_TRY(hipMemset2DAsync(d_dX, (size_t)lddx * h->vsize(), 0, (size_t)k * h->vsize(), (size_t)h->g.n, h->stream));
        else
            HIP_TRY(launch_spmm_reduce_dx(h->comp.at->g, h->comp.at->d, (const uint32_t *)h->comp[A_MAP].ptr, h->value_type, weighted, k,
                                          d_dY, lddy, d_arg, ldarg, d_dX, lddx, h->stream));
    }
    return CSR5HIP_SUCCESS;
}

// Softmax over the stored entries of every row, and its gradient (csr5_softmax.hip): nnz values in CSR order in, nnz out.  They read
// row_ptr and nothing else of the handle, so CSR and CSR5 format are served alike; nothing is allocated or changed: enqueue-only.
int csr5hip_row_softmax(csr5hip_handle h, const void *d_scores_csr, void *d_out_csr)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    const bool loaded = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5;
    const int nnz = loaded ? h->g.nnz : 0;
    if (nnz > 0 && (!d_scores_csr || !d_out_csr))
        return CSR5HIP_INVALID_ARGUMENT;
    if (!loaded)
        return CSR5HIP_UNKOWN_FORMAT;
    if (nnz == 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_row_softmax(h->g.m, h->d.row_ptr, h->value_type, d_scores_csr, d_out_csr, h->stream));
    return CSR5HIP_SUCCESS;
}

int csr5hip_row_softmax_grad(csr5hip_handle h, const void *d_p_csr, const void *d_g_csr, void *d_out_csr)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    const bool loaded = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5;
    const int nnz = loaded ? h->g.nnz : 0;
    if (nnz > 0 && (!d_p_csr || !d_g_csr || !d_out_csr))
        return CSR5HIP_INVALID_ARGUMENT;
    if (!loaded)
        return CSR5HIP_UNKOWN_FORMAT;
    if (nnz == 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_row_softmax_grad(h->g.m, h->d.row_ptr, h->value_type, d_p_csr, d_g_csr, d_out_csr, h->stream));
    return CSR5HIP_SUCCESS;
}

// the dropout fields of a call (p = 0 and head0 = 0 where the call has none): p finite with 0 <= p < 1, head0 >= 0, and every absolute
// head head0 + h an int
static bool att_drop_ok(const AttCall &c)
{
    return std::isfinite(c.p) && c.p >= 0.0 && c.p < 1.0 && c.head0 >= 0 && (long long)c.head0 + (long long)c.heads <= (long long)INT_MAX;
}

// ---- attention on the pattern (csr5_attention*.hip) ---------------------------------------------------------------------------
// The twelve entry points, and the six dropped ones further down, fill a call descriptor (csr5_internal.h) and share ONE path per direction: the checks in ONE order, the
// trivial cases, the launch.  The single-head calls are heads = 1.  The forward reads row_ptr, tile_ptr and the tile-ordered
// column_index of the parent, whatever path spmv() takes (biased: its tile-ordered values too); it allocates nothing and changes
// nothing: enqueue-only.  lowp: the call names the type its operands are stored in (operand_type, judged here); the others take the handle's.
static int attention_forward(csr5hip_handle h, AttVariant variant, bool lowp, int operand_type, const AttCall &c)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (lowp && operand_type != CSR5HIP_BF16 && operand_type != CSR5HIP_F16)
        return CSR5HIP_UNSUPPORTED_VALUE_TYPE;
    if (c.heads < 0 || c.k < 0 || c.d < 0 || !std::isfinite(c.scale) || !std::isfinite(c.negative_slope) || !att_drop_ok(c))
        return CSR5HIP_INVALID_ARGUMENT;
    const long long wk = (long long)c.heads * c.k, wd = (long long)c.heads * c.d;
    if (c.ldq < wk || c.ldk < wk || c.ldv < wd || c.ldo < wd || (c.B && c.ldb < c.heads))
        return CSR5HIP_INVALID_ARGUMENT;
    const int nnz = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5 ? h->g.nnz : 0;
    if (c.heads > 0 && nnz > 0 && ((c.k > 0 && (!c.Q || !c.K)) || (c.d > 0 && !c.V)))
        return CSR5HIP_INVALID_ARGUMENT;
    if (c.heads > 0 && c.d > 0 && h->g.m > 0 && !c.O)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (c.heads == 0 || c.d == 0 || h->g.m <= 0)
        return CSR5HIP_SUCCESS;
    if (lowp && variant == ATT_DROP)
        HIP_TRY(launch_mha_lowp_drop(h->g, h->d, operand_type, c, h->stream));
    else if (lowp)
        HIP_TRY(launch_mha_lowp(h->g, h->d, operand_type, c, h->stream));
    else if (variant == ATT_PLAIN)
        HIP_TRY(launch_mha(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_BIASED)
        HIP_TRY(launch_mha_biased(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_GAT)
        HIP_TRY(launch_gat(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_DROP)
        HIP_TRY(launch_mha_drop(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_DROP_GAT)
        HIP_TRY(launch_gat_drop(h->g, h->d, h->value_type, c, h->stream));
    else
        HIP_TRY(launch_mha_edge(h->g, h->d, h->value_type, c, h->stream));
    return CSR5HIP_SUCCESS;
}

// The backward in two launches: the row kernel on the parent's pattern (it writes dQ, and dS / dB when given), the column kernel on
// the transposed companion's (dK, dV; edge: it finds an entry's rank through the companion's source map, comp[A_MAP], passed, not
// copied).  Allocates nothing, changes nothing of the handle or of its companion: enqueue-only.  c: everything but gt, dt and map,
// which come from the handle.  lowp: as in attention_forward; the operands, the outputs and the zeros of the trivial case are 2-byte
// elements then, the workspace float.
static int attention_backward(csr5hip_handle h, const char *name, AttVariant variant, bool lowp, int operand_type, AttBwdCall c)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (lowp && operand_type != CSR5HIP_BF16 && operand_type != CSR5HIP_F16)
        return CSR5HIP_UNSUPPORTED_VALUE_TYPE;
    if (c.heads < 0 || c.k < 0 || c.d < 0 || !std::isfinite(c.scale) || !std::isfinite(c.negative_slope) || !att_drop_ok(c))
        return CSR5HIP_INVALID_ARGUMENT;
    const long long wk = (long long)c.heads * c.k, wd = (long long)c.heads * c.d;
    if (c.ldq < wk || c.ldk < wk || c.lddq < wk || c.lddk < wk || c.ldv < wd || c.lddo < wd || c.lddv < wd ||
        (c.B && c.ldb < c.heads) || (c.dS && c.ldds < c.heads) || (c.dAr && c.lddar < wk))
        return CSR5HIP_INVALID_ARGUMENT;
    const bool column = c.dK || c.dV; // the column side: needs the workspace and the companion
    const bool any = c.dQ || column || c.dS || c.dAr; // (dAr: gat's second row-side output, null in every other call)
    const int nnz = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5 ? h->g.nnz : 0;
    if (c.heads > 0 && any && nnz > 0 && ((c.k > 0 && (!c.Q || !c.K)) || (c.d > 0 && (!c.V || !c.dO)) || (column && !c.work)))
        return CSR5HIP_INVALID_ARGUMENT;
    if (column && !h->comp.built) {
        g_last_error = std::string(name) + ": dK and dV need the transposed companion, call csr5hip_build_transpose first";
        return CSR5HIP_INVALID_ARGUMENT;
    }
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (!any || c.heads == 0)
        return CSR5HIP_SUCCESS;
    const size_t vs = lowp ? 2 : h->vsize(); // (lowp: the word 0x0000 is +0 in both 16-bit types)
    // no entries (and then no companion arrays, and no element of dS / dB): the zeros
    const bool mapped = variant != ATT_PLAIN && variant != ATT_BIASED; // the column kernel finds B's element through the source map
    if (nnz == 0 || (column && (!h->comp.at || (mapped && !h->comp[A_MAP].ptr)))) {
        if (c.dQ && c.k > 0 && h->g.m > 0)
            HIP_TRY(hipMemset2DAsync(c.dQ, (size_t)c.lddq * vs, 0, (size_t)wk * vs, (size_t)h->g.m, h->stream));
        if (c.dAr && c.k > 0 && h->g.m > 0)
            HIP_TRY(hipMemset2DAsync(c.dAr, (size_t)c.lddar * vs, 0, (size_t)wk * vs, (size_t)h->g.m, h->stream));
        if (c.dK && c.k > 0 && h->g.n > 0)
            HIP_TRY(hipMemset2DAsync(c.dK, (size_t)c.lddk * vs, 0, (size_t)wk * vs, (size_t)h->g.n, h->stream));
        if (c.dV && c.d > 0 && h->g.n > 0)
            HIP_TRY(hipMemset2DAsync(c.dV, (size_t)c.lddv * vs, 0, (size_t)wd * vs, (size_t)h->g.n, h->stream));
        return CSR5HIP_SUCCESS;
    }
    if (column) {
        c.gt = &h->comp.at->g;
        c.dt = &h->comp.at->d;
        c.map = mapped ? (const uint32_t *)h->comp[A_MAP].ptr : nullptr;
    }
    if (lowp && variant == ATT_DROP)
        HIP_TRY(launch_mha_lowp_drop_bwd(h->g, h->d, operand_type, c, h->stream));
    else if (lowp)
        HIP_TRY(launch_mha_lowp_bwd(h->g, h->d, operand_type, c, h->stream));
    else if (variant == ATT_PLAIN)
        HIP_TRY(launch_mha_bwd(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_BIASED)
        HIP_TRY(launch_mha_biased_bwd(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_GAT)
        HIP_TRY(launch_gat_bwd(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_DROP)
        HIP_TRY(launch_mha_drop_bwd(h->g, h->d, h->value_type, c, h->stream));
    else if (variant == ATT_DROP_GAT)
        HIP_TRY(launch_gat_drop_bwd(h->g, h->d, h->value_type, c, h->stream));
    else
        HIP_TRY(launch_mha_edge_bwd(h->g, h->d, h->value_type, c, h->stream));
    return CSR5HIP_SUCCESS;
}

// the descriptors of the entry points' arguments; what a call does not have stays null / 0, the scale 1 (finite)
static AttCall att_call(int heads, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int d, void *O, int ldo)
{
    AttCall c{};
    c.heads = heads; c.k = k; c.d = d; c.scale = 1.0;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.O = O; c.ldo = ldo;
    return c;
}
static AttBwdCall att_bwd_call(int heads, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int d,
                               const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work)
{
    AttBwdCall c{};
    static_cast<AttCall &>(c) = att_call(heads, Q, ldq, K, ldk, k, V, ldv, d, nullptr, 0);
    c.dO = dO; c.lddo = lddo; c.dQ = dQ; c.lddq = lddq; c.dK = dK; c.lddk = lddk; c.dV = dV; c.lddv = lddv; c.work = work;
    return c;
}

int csr5hip_attention(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
                      void *d_O, int ldo)
{
    return attention_forward(h, ATT_PLAIN, false, 0, att_call(1, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo));
}

int csr5hip_attention_backward(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv,
                               int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
                               void *d_work)
{
    const AttBwdCall c = att_bwd_call(1, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    return attention_backward(h, "csr5hip_attention_backward", ATT_PLAIN, false, 0, c);
}

// `heads` heads on packed operands in one launch (the head loop inside the row classes)
int csr5hip_mha(csr5hip_handle h, int heads, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
                void *d_O, int ldo)
{
    return attention_forward(h, ATT_PLAIN, false, 0, att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo));
}

int csr5hip_mha_backward(csr5hip_handle h, int heads, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv,
                         int d, const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
                         void *d_work)
{
    const AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    return attention_backward(h, "csr5hip_mha_backward", ATT_PLAIN, false, 0, c);
}

// the score fma(qk, scale, slopes[h] * value of the entry): reads the parent's tile-ordered values next to its columns (the column
// kernel of the backward: the companion's)
int csr5hip_mha_biased(csr5hip_handle h, int heads, double scale, const void *d_slopes, const void *d_Q, int ldq, const void *d_K, int ldk,
                       int k, const void *d_V, int ldv, int d, void *d_O, int ldo)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.slopes = d_slopes;
    return attention_forward(h, ATT_BIASED, false, 0, c);
}

int csr5hip_mha_biased_backward(csr5hip_handle h, int heads, double scale, const void *d_slopes, const void *d_Q, int ldq, const void *d_K,
                                int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo, void *d_dQ, int lddq,
                                void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dS, int ldds)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.slopes = d_slopes; c.dS = d_dS; c.ldds = ldds;
    return attention_backward(h, "csr5hip_mha_biased_backward", ATT_BIASED, false, 0, c);
}

// the score fma(qk, scale, B[e * ldb + h]), B a caller's tensor in CSR order: reads the parent's pattern and nothing of its values
int csr5hip_mha_edge_bias(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb, const void *d_Q, int ldq, const void *d_K,
                          int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb;
    return attention_forward(h, ATT_EDGE, false, 0, c);
}

// csr5hip_mha_edge_bias on operands stored in bf16 / fp16, computed in float (csr5_attention_lowp.hip): the handle's value type plays
// no part
int csr5hip_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb, const void *d_Q, int ldq,
                     const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb;
    return attention_forward(h, ATT_EDGE, true, operand_type, c);
}

int csr5hip_mha_edge_bias_backward(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb, const void *d_Q, int ldq,
                                   const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                                   void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dB, int lddb)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb;
    return attention_backward(h, "csr5hip_mha_edge_bias_backward", ATT_EDGE, false, 0, c);
}

// csr5hip_mha_edge_bias_backward on operands and gradients stored in bf16 / fp16, computed in float (csr5_attention_bwd_lowp.hip):
// the handle's value type plays no part, and d_work is float whatever it is
int csr5hip_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb, const void *d_Q,
                              int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                              void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dB, int lddb)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb;
    return attention_backward(h, "csr5hip_mha_lowp_backward", ATT_EDGE, true, operand_type, c);
}

// additive attention (csr5hip_gat.h): the edge call's descriptor with the attention vector and the slope; the kernels read the
// parent's pattern and nothing of its values
int csr5hip_gat(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.a = d_a; c.negative_slope = negative_slope;
    return attention_forward(h, ATT_GAT, false, 0, c);
}

int csr5hip_gat_backward(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                         const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO,
                         int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dB, int lddb,
                         void *d_dAr, int lddar)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb; c.a = d_a; c.negative_slope = negative_slope;
    c.dAr = d_dAr; c.lddar = lddar;
    return attention_backward(h, "csr5hip_gat_backward", ATT_GAT, false, 0, c);
}

// the dropped calls (csr5hip_dropout.h): the edge call's and the additive one's descriptors with the mask's fields; the shared paths
// above judge them and launch the dropped kernels
static void att_set_dropout(AttCall &c, double p, unsigned long long seed, unsigned long long offset, int head0)
{
    c.p = p; c.seed = seed; c.offset = offset; c.head0 = head0;
}

int csr5hip_dropout_mha(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb, const void *d_Q, int ldq, const void *d_K,
                        int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo, double p, unsigned long long seed,
                        unsigned long long offset, int head0)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_forward(h, ATT_DROP, false, 0, c);
}

int csr5hip_dropout_mha_backward(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb, const void *d_Q, int ldq,
                                 const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                                 void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work, void *d_dB, int lddb,
                                 double p, unsigned long long seed, unsigned long long offset, int head0)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_backward(h, "csr5hip_dropout_mha_backward", ATT_DROP, false, 0, c);
}

// the same two on operands stored in bf16 / fp16 (csr5hip_dropout_lowp.h): the pair (ATT_DROP, lowp) picks the 16-bit dropped kernels
int csr5hip_dropout_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb, const void *d_Q,
                             int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo, double p,
                             unsigned long long seed, unsigned long long offset, int head0)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_forward(h, ATT_DROP, true, operand_type, c);
}

int csr5hip_dropout_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
                                      const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
                                      const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
                                      void *d_work, void *d_dB, int lddb, double p, unsigned long long seed, unsigned long long offset,
                                      int head0)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_backward(h, "csr5hip_dropout_mha_lowp_backward", ATT_DROP, true, operand_type, c);
}

int csr5hip_dropout_gat(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo,
                        double p, unsigned long long seed, unsigned long long offset, int head0)
{
    AttCall c = att_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_O, ldo);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.a = d_a; c.negative_slope = negative_slope;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_forward(h, ATT_DROP_GAT, false, 0, c);
}

int csr5hip_dropout_gat_backward(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B,
                                 int ldb, const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
                                 const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
                                 void *d_work, void *d_dB, int lddb, void *d_dAr, int lddar, double p, unsigned long long seed,
                                 unsigned long long offset, int head0)
{
    AttBwdCall c = att_bwd_call(heads, d_Q, ldq, d_K, ldk, k, d_V, ldv, d, d_dO, lddo, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_work);
    c.scale = scale; c.B = d_B; c.ldb = ldb; c.dS = d_dB; c.ldds = lddb; c.a = d_a; c.negative_slope = negative_slope;
    c.dAr = d_dAr; c.lddar = lddar;
    att_set_dropout(c, p, seed, offset, head0);
    return attention_backward(h, "csr5hip_dropout_gat_backward", ATT_DROP_GAT, false, 0, c);
}

// the mask itself: it needs only nnz, so CSR and CSR5 format are served alike; enqueue-only
int csr5hip_dropout_mask(csr5hip_handle h, int heads, double p, unsigned long long seed, unsigned long long offset, int head0,
                         void *d_mask, int ldm)
{
    AttCall c{};
    c.heads = heads;
    att_set_dropout(c, p, seed, offset, head0);
    if (!h || heads < 0 || !att_drop_ok(c) || ldm < heads)
        return CSR5HIP_INVALID_ARGUMENT;
    const bool loaded = h->format == CSR5HIP_FORMAT_CSR || h->format == CSR5HIP_FORMAT_CSR5;
    const int nnz = loaded ? h->g.nnz : 0;
    if (nnz > 0 && heads > 0 && !d_mask)
        return CSR5HIP_INVALID_ARGUMENT;
    if (!loaded)
        return CSR5HIP_UNKOWN_FORMAT;
    if (nnz == 0 || heads == 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_dropout_mask(nnz, c, (unsigned char *)d_mask, ldm, h->stream));
    return CSR5HIP_SUCCESS;
}

// ---- new values under an unchanged pattern (csr5_refresh.hip) ---------------------------------------------------------------
// The source map of the slab child, built from the parent's tile-ordered column_index: one allocation for the map, one -- released
// again -- for the sort's temporaries, one synchronisation.  Nothing of the handle is modified before the map is complete.
static int build_refresh_map(csr5hip_handle h)
{
    const Geometry &g = h->g;
    const csr5hip_handle c = h->slab.child;
    if (stream_is_capturing(h->stream)) {
        g_last_error = "csr5hip_update_values: the first call after a conversion builds the slab child's source map and cannot be "
                       "captured: call it once outside the capture";
        return CSR5HIP_HIP_ERROR;
    }
    size_t tmp_bytes = 0;
    hipError_t e = refresh_map_tmp_bytes(g.nnz, c->d.slab_bits, &tmp_bytes);
    Buffer tmp;
    if (e == hipSuccess)
        e = h->slab[B_REFRESH_MAP].reserve((size_t)g.nnz * 4);
    if (e == hipSuccess)
        e = tmp.reserve(tmp_bytes);
    if (e == hipSuccess)
        e = refresh_build_map(g, h->d, c->d.slab_bits, c->d.slab_shift, tmp.ptr, tmp_bytes, (uint32_t *)h->slab[B_REFRESH_MAP].ptr, h->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    tmp.release();
    if (e != hipSuccess) {
        (void)hipGetLastError(); // (clear the sticky allocation error: the handle stays usable with its old values)
        h->slab[B_REFRESH_MAP].release();
        return fail_hip(e, "csr5hip_update_values: source map of the slab child");
    }
    h->slab.refresh_map_valid = true;
    return CSR5HIP_SUCCESS;
}

static int update_values_self(csr5hip_handle h, const void *d_val_csr);

// With a transposed companion the same call gives it the new values too: gathered through the source map into the staging buffer
// (A^T's CSR order), then the companion's own refresh, on the same stream behind the parent's.  Whatever cannot be enqueued -- the
// source map of the companion's slab child, built by its first update -- is done BEFORE anything is changed.
int csr5hip_update_values(csr5hip_handle h, const void *d_val_csr)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    csr5hip_handle t = h->format == CSR5HIP_FORMAT_CSR5 ? h->comp.at : nullptr;
    if (!t || !d_val_csr)
        return update_values_self(h, d_val_csr);
    if (t->slab.S > 0 && !t->slab.refresh_map_valid) {
        const int rc = build_refresh_map(t);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
    }
    int rc = update_values_self(h, d_val_csr);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    HIP_TRY(companion_gather(h->g.nnz, (int)h->vsize(), (const uint32_t *)h->comp[A_MAP].ptr, d_val_csr, h->comp[A_STAGE].ptr, h->stream));
    return update_values_self(t, h->comp[A_STAGE].ptr);
}

static int update_values_self(csr5hip_handle h, const void *d_val_csr)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format != CSR5HIP_FORMAT_CSR && h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (h->g.nnz == 0)
        return CSR5HIP_SUCCESS;
    if (!d_val_csr)
        return CSR5HIP_INVALID_ARGUMENT;
    const size_t bytes = (size_t)h->g.nnz * h->vsize();
    {
        const uintptr_t a = (uintptr_t)d_val_csr, v = (uintptr_t)h->d.val;
        if (a < v + bytes && v < a + bytes) {
            g_last_error = "csr5hip_update_values: d_val_csr overlaps the value array given to inputCSR (the handle keeps that array "
                           "in its own order)";
            return CSR5HIP_INVALID_ARGUMENT;
        }
    }
    hipStream_t s = h->stream;
    if (h->format == CSR5HIP_FORMAT_CSR) {
        HIP_TRY(hipMemcpyAsync(h->d.val, d_val_csr, bytes, hipMemcpyDeviceToDevice, s));
        return CSR5HIP_SUCCESS;
    }
    const csr5hip_handle c = h->slab.S > 0 ? h->slab.child : nullptr;
    // the fp32 copy of a hot child's values is re-decided as the slab build decides it (narrow_child_values): one host synchronisation
    const bool renarrow = c && c->hot_enabled && h->req.narrow && h->value_type == CSR5HIP_F64;
    if (renarrow && stream_is_capturing(s)) {
        g_last_error = "csr5hip_update_values: CSR5HIP_OPT_NARROW_VALUES re-checks the values on the host and cannot be captured";
        return CSR5HIP_HIP_ERROR;
    }
    if (c && !h->slab.refresh_map_valid) {
        const int rc = build_refresh_map(h);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
    }
    HIP_TRY(launch_refresh_values(h->g, h->d.tile_ptr, h->value_type, false, nullptr, d_val_csr, h->d.val, s));
    if (!c)
        return CSR5HIP_SUCCESS;
    HIP_TRY(launch_refresh_values(c->g, c->d.tile_ptr, c->value_type, c->hot_enabled, (const uint32_t *)h->slab[B_REFRESH_MAP].ptr,
                                  d_val_csr, c->d.val, s));
    if (!renarrow)
        return CSR5HIP_SUCCESS;
    bool narrow = false, copying = false;
    const hipError_t e = narrow_child_values(h, c, false, &narrow, &copying); // (the copy is enqueued, not waited for)
    if (e != hipSuccess && !copying)
        return fail_hip(e, "csr5hip_update_values: fp32 exactness test of the values");
    if (e != hipSuccess) { // the copy is an optional accelerator: the fp64 values serve
        (void)hipGetLastError();
        set_last_error(std::string("csr5hip_update_values: fp32 copy of the values not built: ") + hipGetErrorString(e));
    }
    if (narrow != h->slab.values_narrowed) {
        // another instantiation of the range kernel from here on: its LDS limit, and no graph recorded so far may be replayed
        c->d.val32 = narrow ? (const float *)h->slab[B_VAL32].ptr : nullptr;
        h->slab.values_narrowed = narrow;
        h->drop_graphs();
        HIP_TRY(prepare_spmv_hot(c->g, c->d, c->value_type, c->opt));
    }
    return CSR5HIP_SUCCESS;
}

// ---- transposed companion (csr5_companion.hip) --------------------------------------------------------------------------------
// The CSR of A^T and its source map from the parent's tile-ordered arrays, then an ordinary conversion of a handle of shape (n, m)
// that carries the parent's value type, stream, sigma request and options.  Nothing of the parent is modified.
// What a transposed companion has of its parent's options: EVERYTHING, but for the snapshot of x.  (A slab child,
// csr5_slab_build.hip inherit_child, is the opposite: it takes only the mode and two requests and keeps defaults for the rest.)
static void inherit_companion(csr5hip_handle t, const csr5hip_handle_s *h)
{
    t->req = h->req;
    t->req.x_snapshot = 0; // spmv_t takes x per call: always read live
    t->opt.mode = h->opt.mode;
    t->opt.xcd_remap = h->opt.xcd_remap;
}

static int build_companion(csr5hip_handle h)
{
    const Geometry &g = h->g;
    hipStream_t s = h->stream;
    const size_t vs = h->vsize();
    size_t tmp_bytes = 0;
    Buffer tmp;
    hipError_t e = companion_tmp_bytes(g.n, g.nnz, &tmp_bytes);
    if (e == hipSuccess)
        e = h->comp[A_ROW_PTR].reserve(((size_t)g.n + 1) * 4);
    if (e == hipSuccess)
        e = h->comp[A_COL].reserve((size_t)g.nnz * 4);
    if (e == hipSuccess)
        e = h->comp[A_VAL].reserve((size_t)g.nnz * vs);
    if (e == hipSuccess)
        e = h->comp[A_MAP].reserve((size_t)g.nnz * 4);
    if (e == hipSuccess)
        e = h->comp[A_STAGE].reserve((size_t)g.nnz * vs);
    if (e == hipSuccess)
        e = tmp.reserve(tmp_bytes);
    if (e == hipSuccess)
        e = companion_build(g, h->d, (int)vs, tmp.ptr, tmp_bytes, (int32_t *)h->comp[A_ROW_PTR].ptr, (int32_t *)h->comp[A_COL].ptr,
                            h->comp[A_VAL].ptr, (uint32_t *)h->comp[A_MAP].ptr, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    tmp.release();
    if (e != hipSuccess) {
        (void)hipGetLastError(); // (clear the sticky allocation error: the parent stays usable)
        return fail_hip(e, "csr5hip_build_transpose: CSR of the transposed matrix");
    }
    csr5hip_handle t = new csr5hip_handle_s();
    h->comp.at = t;
    t->g.m = g.n;
    t->g.n = g.m;
    t->value_type = h->value_type;
    t->stream = s;
    inherit_companion(t, h);
    int rc = csr5hip_input_csr(t, g.nnz, (int32_t *)h->comp[A_ROW_PTR].ptr, (int32_t *)h->comp[A_COL].ptr, h->comp[A_VAL].ptr);
    t->sigma_auto = h->sigma_auto;
    t->sigma_request = h->sigma_auto || h->sigma_request < CSR5HIP_MIN_SIGMA ? csr5hip_auto_sigma(t->g.m, g.nnz, t->value_type)
                                                                              : h->sigma_request;
    if (rc == CSR5HIP_SUCCESS)
        rc = csr5hip_as_csr5(t);
    return rc;
}

int csr5hip_build_transpose(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (h->comp.built)
        return CSR5HIP_SUCCESS;
    if (h->g.nnz == 0) { // nothing to hold: spmv_t applies the empty-row contract to all n rows
        h->comp.built = true;
        return CSR5HIP_SUCCESS;
    }
    if (stream_is_capturing(h->stream)) {
        g_last_error = "csr5hip_build_transpose allocates and synchronises and cannot be captured: call it outside the capture";
        return CSR5HIP_HIP_ERROR;
    }
    const double t0 = now_ms();
    const int rc = build_companion(h);
    if (rc != CSR5HIP_SUCCESS) {
        const std::string why = g_last_error;
        (void)hipGetLastError();
        h->comp.release();
        g_last_error = why;
        return rc;
    }
    h->comp.built = true;
    h->comp.t_build = now_ms() - t0;
    return CSR5HIP_SUCCESS;
}

static int companion_ready(csr5hip_handle h, const char *who)
{
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (!h->comp.built) {
        g_last_error = std::string(who) + ": no transposed companion, call csr5hip_build_transpose first";
        return CSR5HIP_INVALID_ARGUMENT;
    }
    return CSR5HIP_SUCCESS;
}

// y = A^T x: one spmv() of the companion with the caller's x, on whatever path its conversion selected
int csr5hip_spmv_t(csr5hip_handle h, const void *d_x, void *d_y)
{
    if (!h || !d_x || !d_y)
        return CSR5HIP_INVALID_ARGUMENT;
    const int rc = companion_ready(h, "csr5hip_spmv_t");
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    csr5hip_handle t = h->comp.at;
    if (!t) { // nnz = 0: every row of A^T is an empty row in front of the tail
        if (h->req.zero_empty && h->g.n > 0)
            HIP_TRY(hipMemsetAsync(d_y, 0, (size_t)h->g.n * h->vsize(), h->stream));
        return CSR5HIP_SUCCESS;
    }
    t->x = d_x; // (the companion records no graphs of its own and keeps no snapshot: nothing to invalidate)
    HIP_TRY(enqueue_spmv(t, d_y, t->stream, false));
    return CSR5HIP_SUCCESS;
}

// Y = A^T X: csr5hip_spmm of the companion
int csr5hip_spmm_t(csr5hip_handle h, const void *d_X, int ldx, int k, void *d_Y, int ldy)
{
    if (!h || k < 0 || ldx < k || ldy < k || (k > 0 && (!d_X || !d_Y)))
        return CSR5HIP_INVALID_ARGUMENT;
    const int rc = companion_ready(h, "csr5hip_spmm_t");
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    if (h->comp.at)
        return csr5hip_spmm(h->comp.at, d_X, ldx, k, d_Y, ldy);
    if (k > 0) { // nnz = 0
        Geometry gt{};
        gt.m = h->g.n;
        gt.n = h->g.m;
        HIP_TRY(launch_spmm(gt, DeviceArrays{}, h->value_type, d_X, ldx, k, d_Y, ldy, nullptr, h->req.zero_empty, 0, h->stream));
    }
    return CSR5HIP_SUCCESS;
}

int csr5hip_snapshot_x(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format != CSR5HIP_FORMAT_CSR5 || !h->x)
        return CSR5HIP_SUCCESS; // (nothing to copy yet: the first spmv() after asCSR5 / setX takes it)
    HIP_TRY(ensure_x_snapshot(h, h->stream));
    return CSR5HIP_SUCCESS;
}

int csr5hip_spmv_repeat(csr5hip_handle h, double alpha, void *d_y, int count)
{
    if (!h || !d_y || count < 0)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format == CSR5HIP_FORMAT_CSR)
        return CSR5HIP_UNSUPPORTED_CSR_SPMV;
    if (h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (!h->x)
        return CSR5HIP_INVALID_ARGUMENT;
    if (count == 0)
        return CSR5HIP_SUCCESS;
    HIP_TRY(ensure_x_snapshot(h, h->stream));
    GraphKey key{d_y, count, h->opt.mode};
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        // capture on a private stream so the caller's stream state is untouched
        hipStream_t cs = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        int rc = CSR5HIP_SUCCESS;
        if (e == hipSuccess) {
            for (int i = 0; i < count && e == hipSuccess; i++)
                e = enqueue_spmv(h, d_y, cs, true);
            hipError_t e2 = hipStreamEndCapture(cs, &graph);
            if (e == hipSuccess)
                e = e2;
        }
        hipGraphExec_t exec = nullptr;
        if (e == hipSuccess)
            e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph)
            (void)hipGraphDestroy(graph);
        (void)hipStreamDestroy(cs);
        if (e != hipSuccess)
            rc = fail_hip(e, "hipGraph capture of spmv");
        if (rc != CSR5HIP_SUCCESS)
            return rc;
        if (h->graphs.size() >= 8)
            h->drop_graphs();
        it = h->graphs.emplace(key, exec).first;
    }
    HIP_TRY(hipGraphLaunch(it->second, h->stream));
    (void)alpha;
    return CSR5HIP_SUCCESS;
}

int csr5hip_spmv_rotate(csr5hip_handle *hs, void **d_ys, int k, double alpha, int count)
{
    (void)alpha;
    if (!hs || !d_ys || k < 1 || count < 0)
        return CSR5HIP_INVALID_ARGUMENT;
    for (int i = 0; i < k; i++) {
        if (!hs[i] || !d_ys[i] || !hs[i]->x)
            return CSR5HIP_INVALID_ARGUMENT;
        if (hs[i]->format == CSR5HIP_FORMAT_CSR)
            return CSR5HIP_UNSUPPORTED_CSR_SPMV;
        if (hs[i]->format != CSR5HIP_FORMAT_CSR5)
            return CSR5HIP_UNKOWN_FORMAT;
    }
    if (count == 0)
        return CSR5HIP_SUCCESS;
    csr5hip_handle h0 = hs[0];
    for (int i = 0; i < k; i++) {
        // every handle's snapshot on its OWN stream (a later spmv(hs[i]) there is ordered behind it); the rotating graph,
        // launched on hs[0]'s stream, waits for the foreign ones
        const bool pending = hs[i]->req.x_snapshot && !hs[i]->slab.xperm_valid;
        HIP_TRY(ensure_x_snapshot(hs[i], hs[i]->stream));
        if (pending && hs[i]->stream != h0->stream) {
            hipEvent_t ev = nullptr;
            HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            hipError_t e = hipEventRecord(ev, hs[i]->stream);
            if (e == hipSuccess)
                e = hipStreamWaitEvent(h0->stream, ev, 0);
            (void)hipEventDestroy(ev);
            HIP_TRY(e);
        }
    }
    std::vector<void *> key;
    key.push_back((void *)(intptr_t)count);
    for (int i = 0; i < k; i++) {
        key.push_back(hs[i]);
        key.push_back(d_ys[i]);
        // the graph bakes in every handle's x, format arrays and slab buffers: any change of handle i (set_x, set_option,
        // asCSR / asCSR5, set_stream) bumps its generation and must invalidate the graph cached on hs[0]
        key.push_back((void *)(uintptr_t)hs[i]->generation);
    }
    if (!h0->rotate_exec || h0->rotate_key != key) {
        if (h0->rotate_exec)
            (void)hipGraphExecDestroy(h0->rotate_exec);
        h0->rotate_exec = nullptr;
        h0->rotate_key.clear();
        hipStream_t cs = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        hipGraph_t graph = nullptr;
        hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
        if (e == hipSuccess) {
            for (int i = 0; i < count && e == hipSuccess; i++)
                e = enqueue_spmv(hs[i % k], d_ys[i % k], cs, true);
            hipError_t e2 = hipStreamEndCapture(cs, &graph);
            if (e == hipSuccess)
                e = e2;
        }
        hipGraphExec_t exec = nullptr;
        if (e == hipSuccess)
            e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (graph)
            (void)hipGraphDestroy(graph);
        (void)hipStreamDestroy(cs);
        if (e != hipSuccess)
            return fail_hip(e, "hipGraph capture of rotating spmv");
        h0->rotate_exec = exec;
        h0->rotate_key = key;
    }
    HIP_TRY(hipGraphLaunch(h0->rotate_exec, h0->stream));
    return CSR5HIP_SUCCESS;
}

// Measured sigma selection: what the reference's per-architecture
// (r, s, t, u) tables (anonymouslib_cuda.h:297-313, anonymouslib_opencl.h:341-357) approximate, done on
// the matrix itself.  For every candidate sigma: CSR -> CSR5, a few warm SpMVs, then `reps` SpMVs
// replayed from one hipGraph and timed with HIP events; the fastest sigma stays converted.
int csr5hip_autotune_sigma(csr5hip_handle h, void *d_y, int *best_sigma, double *best_us)
{
    if (!h || !d_y)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format != CSR5HIP_FORMAT_CSR && h->format != CSR5HIP_FORMAT_CSR5)
        return CSR5HIP_UNKOWN_FORMAT;
    if (!h->x)
        return CSR5HIP_INVALID_ARGUMENT;
    int rc = csr5hip_as_csr(h);
    if (rc != CSR5HIP_SUCCESS)
        return rc;
    static const int candidates[] = {4, 5, 6, 8, 10, 12, 16, 20, 24, 32};
    int best = 0;
    // the slab child that served the last timed candidate: (slabs, hot table, child sigma); a later candidate that converts
    // to the SAME child -- the child's sigma is capped, so every larger parent sigma may -- would time the same kernel again
    int timed_S = -1, timed_hot = -1, timed_child_sigma = -1;
    double best_ms = 1e300;
    for (int sigma : candidates) {
        if ((long long)OMEGA * sigma > (long long)h->g.nnz && sigma != 4)
            continue; // fewer non-zeros than one tile: nothing to choose
        h->sigma_request = sigma;
        h->sigma_auto = false;
        rc = csr5hip_as_csr5(h);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
        // The slab decision itself depends on the parent's sigma (tile count, x-window coverage): only a candidate that
        // was CONVERTED and produced the child already timed is skipped.
        if (h->slab.S > 0 && h->slab.child && h->slab.child->hot_enabled) {
            const int cs = h->slab.child->g.sigma;
            if (h->slab.S == timed_S && timed_hot == 1 && cs == timed_child_sigma) {
                rc = csr5hip_as_csr(h);
                if (rc != CSR5HIP_SUCCESS)
                    return rc;
                continue;
            }
            timed_S = h->slab.S, timed_hot = 1, timed_child_sigma = cs;
        } else {
            timed_S = timed_hot = timed_child_sigma = -1;
        }
        for (int i = 0; i < 3 && rc == CSR5HIP_SUCCESS; i++)
            rc = csr5hip_spmv(h, 1.0, d_y);
        // size the timed batch to ~0.5 ms from one timed probe launch
        double probe_ms = 0;
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_timer_start(h);
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_spmv(h, 1.0, d_y);
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_timer_stop(h, &probe_ms);
        int reps = probe_ms > 0 ? (int)(0.5 / probe_ms) : 50;
        reps = reps < 5 ? 5 : (reps > 200 ? 200 : reps);
        double ms = 0;
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_spmv_repeat(h, 1.0, d_y, reps); // instantiate + warm
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_timer_start(h);
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_spmv_repeat(h, 1.0, d_y, reps);
        if (rc == CSR5HIP_SUCCESS) rc = csr5hip_timer_stop(h, &ms);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
        ms /= reps;
        if (ms < best_ms) {
            best_ms = ms;
            best = sigma;
        }
        rc = csr5hip_as_csr(h);
        if (rc != CSR5HIP_SUCCESS)
            return rc;
    }
    h->sigma_auto = !best;
    if (!best)
        best = csr5hip_auto_sigma(h->g.m, h->g.nnz, h->value_type);
    h->sigma_request = best;
    rc = csr5hip_as_csr5(h);
    if (best_sigma) *best_sigma = best;
    if (best_us) *best_us = best_ms * 1e3;
    return rc;
}

int csr5hip_get_info(csr5hip_handle h, csr5hip_info *info)
{
    if (!h || !info)
        return CSR5HIP_INVALID_ARGUMENT;
    memset(info, 0, sizeof(*info));
    info->format = h->format;
    info->m = h->g.m;
    info->n = h->g.n;
    info->nnz = h->g.nnz;
    info->value_type = h->value_type;
    info->omega = OMEGA;
    info->sigma = h->format == CSR5HIP_FORMAT_CSR5 ? h->g.sigma : h->sigma_request;
    if (h->format == CSR5HIP_FORMAT_CSR5) {
        info->bit_y_offset = h->g.bit_y;
        info->bit_scansum_offset = BIT_SS;
        info->num_packet = h->g.num_packet;
        info->p = h->g.p;
        info->tail_partition_start = h->g.tail_start;
        info->num_offsets = h->num_offsets;
        info->d_tile_ptr = h->d.tile_ptr;
        info->d_tile_desc = h->d.tile_desc;
        info->d_offset_ptr = h->d.offset_ptr;
        info->d_offset = h->d.offset;
    }
    info->x_window_tiles = h->xwin_tiles;
    info->x_window_lines = h->xwin_tiles > 0 ? (int)(h->xwin_lines / h->xwin_tiles) : 0;
    info->x_window_cover_pct = h->g.p > 1 ? (int)(h->xwin_covered * 100 / ((long long)(h->g.p - 1) * h->g.tile_elems)) : 0;
    info->x_window_active = h->opt.x_window && h->opt.mode == 1 ? 1 : 0; // the two-pass kernel has no x-window variant
    info->t_malloc_ms = h->t_malloc;
    info->t_tile_ptr_ms = h->t_tile_ptr;
    info->t_tile_desc_ms = h->t_tile_desc;
    info->t_transpose_ms = h->t_transpose;
    info->column_slabs = h->slab.S;
    info->slab_shift = h->req.slab_shift;
    info->slab_segments = h->slab.m2;
    info->slab_sigma = h->slab.S > 0 ? h->slab.child->g.sigma : 0;
    info->slab_tiles = h->slab.S > 0 ? h->slab.child->g.p : 0;
    info->t_slab_ms = h->slab.t_slab;
    info->slab_hot = h->slab.S > 0 && h->slab.child->hot_enabled ? 1 : 0;
    info->slab_hot_cover_pct = h->slab.hot_cover_pct;
    info->slab_fallback = h->slab.fallback ? 1 : 0;
    info->slab_x_permuted = h->slab.S > 0 && h->slab.child->hot_enabled ? 1 : 0;
    info->slab_cold_entries = info->slab_x_permuted ? h->slab.cold_total : 0;
    info->x_snapshot = h->req.x_snapshot;
    info->slab_values_narrowed = h->slab.S > 0 && h->slab.values_narrowed ? 1 : 0;
    info->carries_deferred = h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0 && h->g.defer ? 1 : 0;
    info->narrow_columns = h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0 && h->opt.col16 && h->opt.x_window && h->opt.mode == 1 ? 1 : 0;
    info->flagged_columns = h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0 && h->opt.col31 && !h->opt.x_window && h->opt.mode == 1 ? 1 : 0;
    // the kernel variants launch_sigma() picks: compile-time sigma 4..32 only (the run-time-sigma kernel has neither)
    const bool plain_ct = h->format == CSR5HIP_FORMAT_CSR5 && h->slab.S <= 0 && h->g.sigma >= 4 && h->g.sigma <= CSR5HIP_MAX_SIGMA;
    info->lds_y = plain_ct && h->opt.lds_y && (size_t)OMEGA * h->g.sigma * h->vsize() <= 8192 ? 1 : 0;
    info->stream_nt = plain_ct && h->opt.stream_nt && h->opt.mode == 1 && !h->opt.x_window ? 1 : 0;
    long long bytes = (long long)(h->b_arena.cap + h->b_col16.cap + h->b_col31.cap) + h->slab.bytes();
    info->transpose_built = h->comp.built ? 1 : 0;
    info->t_transpose_build_ms = h->comp.t_build;
    if (h->comp.at) {
        csr5hip_info ti;
        csr5hip_get_info(h->comp.at, &ti);
        info->t_sigma = ti.sigma;
        info->t_p = ti.p;
        info->t_tail_partition_start = ti.tail_partition_start;
        info->t_column_slabs = ti.column_slabs;
        info->t_slab_hot = ti.slab_hot;
        info->t_x_window_active = ti.x_window_active;
        bytes += ti.device_bytes + h->comp.bytes();
    } else if (h->comp.built) { // nnz = 0: what a handle of the empty n x m matrix reports
        info->t_sigma = h->sigma_auto ? csr5hip_auto_sigma(h->g.n, 0, h->value_type) : h->sigma_request;
        info->t_tail_partition_start = h->g.n;
    }
    info->device_bytes = bytes;
    return CSR5HIP_SUCCESS;
}

// borrowed pointers of the hot slab child, for tests and inspection: nothing is launched, copied or allocated
int csr5hip_get_slab_view(csr5hip_handle h, csr5hip_slab_view *out)
{
    if (!h || !out)
        return CSR5HIP_INVALID_ARGUMENT;
    const csr5hip_handle_s *c = h->slab.child;
    if (h->format != CSR5HIP_FORMAT_CSR5 || h->slab.S <= 0 || !c || !c->hot_enabled) {
        set_last_error("csr5hip_get_slab_view: the handle has no column-slab child with a hot table (csr5hip_info.slab_hot == 0)");
        return CSR5HIP_INVALID_ARGUMENT;
    }
    csr5hip_slab_view v{};
    v.S = h->slab.S;
    v.capacity = c->d.hot_capacity;
    v.slab_shift = c->d.slab_shift;
    v.slab_bits = c->d.slab_bits;
    v.sigma = c->g.sigma;
    v.T = c->g.tile_elems;
    v.p = c->g.p;
    v.tail_start = c->g.tail_start;
    v.segments = c->g.m;
    v.cold_total = c->d.cold_total;
    v.stride = h->slab.sample_stride;
    v.min_count = h->slab.min_count;
    v.values_narrowed = h->slab.values_narrowed ? 1 : 0;
    v.slab_off = c->d.slab_off;
    v.hot_tile0 = c->d.hot_tile0;
    v.hot_count = c->d.hot_count;
    v.hot_cols = c->d.hot_cols;
    v.cold_base = c->d.cold_base;
    v.cold_cols = c->d.cold_cols;
    v.col_lo = c->d.col_lo;
    v.col_hi = c->d.col_hi;
    v.row_ptr = c->d.row_ptr;
    v.col = c->d.col;
    v.val = c->d.val;
    v.val32 = h->slab.values_narrowed ? c->d.val32 : nullptr;
    v.tile_ptr = c->d.tile_ptr;
    v.range_begin = c->d.range_begin;
    // (the prefix costs lie behind the cut table in the same buffer)
    v.range_cost = reinterpret_cast<const unsigned long long *>(reinterpret_cast<const char *>(c->d.range_begin) +
                                                                range_cut_layout(v.S, v.p - 1).prefix);
    v.range_head = c->d.range_head;
    v.xperm = c->d.xperm;
    *out = v;
    return CSR5HIP_SUCCESS;
}

// ---- device shims ---------------------------------------------------------------------------
int csr5hip_device_count(int *count)
{
    if (!count)
        return CSR5HIP_INVALID_ARGUMENT;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        *count = 0;
        return fail_hip(e, "hipGetDeviceCount");
    }
    return CSR5HIP_SUCCESS;
}

int csr5hip_set_device(int device)
{
    HIP_TRY(hipSetDevice(device));
    return CSR5HIP_SUCCESS;
}

int csr5hip_device_name(int device, char *buf, size_t buflen, double *clock_mhz)
{
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (buf && buflen) {
        // the marketing name comes from libdrm's amdgpu.ids and is empty where that file is missing:
        // fall back to the architecture string (gfx950:...)
        strncpy(buf, prop.name[0] ? prop.name : prop.gcnArchName, buflen - 1);
        buf[buflen - 1] = 0;
    }
    if (clock_mhz)
        *clock_mhz = prop.clockRate * 1e-3;
    return CSR5HIP_SUCCESS;
}

int csr5hip_malloc(void **dptr, size_t bytes)
{
    if (!dptr)
        return CSR5HIP_INVALID_ARGUMENT;
    HIP_TRY(hipMalloc(dptr, bytes ? bytes : 4));
    return CSR5HIP_SUCCESS;
}

int csr5hip_device_free(void *dptr)
{
    HIP_TRY(hipFree(dptr));
    return CSR5HIP_SUCCESS;
}

int csr5hip_memcpy_h2d(void *dst, const void *src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return CSR5HIP_SUCCESS;
}

int csr5hip_memcpy_d2h(void *dst, const void *src, size_t bytes)
{
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return CSR5HIP_SUCCESS;
}

int csr5hip_memset(void *dptr, int value, size_t bytes)
{
    HIP_TRY(hipMemset(dptr, value, bytes));
    return CSR5HIP_SUCCESS;
}

int csr5hip_synchronize(void)
{
    HIP_TRY(hipDeviceSynchronize());
    return CSR5HIP_SUCCESS;
}

int csr5hip_timer_start(csr5hip_handle h)
{
    if (!h)
        return CSR5HIP_INVALID_ARGUMENT;
    if (!h->ev0) {
        HIP_TRY(hipEventCreate(&h->ev0));
        HIP_TRY(hipEventCreate(&h->ev1));
    }
    HIP_TRY(hipEventRecord(h->ev0, h->stream));
    return CSR5HIP_SUCCESS;
}

int csr5hip_timer_stop(csr5hip_handle h, double *ms)
{
    if (!h || !ms || !h->ev0)
        return CSR5HIP_INVALID_ARGUMENT;
    HIP_TRY(hipEventRecord(h->ev1, h->stream));
    HIP_TRY(hipEventSynchronize(h->ev1));
    float f = 0;
    HIP_TRY(hipEventElapsedTime(&f, h->ev0, h->ev1));
    *ms = f;
    return CSR5HIP_SUCCESS;
}

} // extern "C"
