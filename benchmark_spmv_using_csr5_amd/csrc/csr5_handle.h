// csr5_handle.h -- the handle behind the C ABI and what the host units of libcsr5hip.so share (csr5_capi.hip, csr5_convert.hip,
// csr5_checkpoint.hip, csr5_slab_build.hip).  No kernel unit includes it.  Nothing declared here is an exported symbol.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "csr5_internal.h"
#pragma GCC visibility push(hidden) // (its inline functions stay inside the library too)
#include "csr5_slab_plan.h"
#pragma GCC visibility pop

namespace csr5 {
void set_last_error(const std::string &msg); // (csr5_ingest.hip and csr5_multi.hip use it too: the one name here that stays visible)
} // namespace csr5

#pragma GCC visibility push(hidden)
namespace csr5 {

const std::string &last_error();
int fail_hip(hipError_t e, const char *what); // records "<what>: <HIP's text>", returns CSR5HIP_HIP_ERROR

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail_hip(e_, #expr);                                                            \
    } while (0)

struct Buffer {
    void *ptr = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        if (ptr) {
            hipError_t e = hipFree(ptr);
            if (e != hipSuccess)
                return e;
            ptr = nullptr;
            cap = 0;
        }
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e == hipSuccess)
            cap = bytes;
        return e;
    }
    void release()
    {
        if (ptr)
            (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

struct GraphKey {
    void *y;
    int count;
    int mode;
    bool operator==(const GraphKey &o) const { return y == o.y && count == o.count && mode == o.mode; }
};
struct GraphKeyHash {
    size_t operator()(const GraphKey &k) const
    {
        return std::hash<void *>()(k.y) ^ (size_t)k.count * 1000003u ^ (size_t)k.mode * 7919u;
    }
};

inline double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---- column slabs (csr5_slab.hip, built by csr5_slab_build.hip): the stacked matrix lives in an internal child handle ----
// Every device buffer of the structure, ONE list: release(), bytes() and the builder all go through it.
enum SlabBuf {
    B_ROW_PTR2, B_COL2, B_VAL2, B_VAL32, B_P, B_ROWIDX, B_BASE, B_NONEMPTY,
    B_TMP, // temporaries of the slab build; kept between conversions only while small (SLAB_TMP_KEEP)
    // LDS hot table of the slab child (k_spmv_range): chosen at conversion, see csr5_slab.hip
    B_HOT_COLS, B_HOT_COUNT, B_HOT_TILE0, B_SLAB_OFF, B_LEAD, B_RANGE_HEAD, B_RANGE_CUT,
    B_COL_LO, B_COL_HI, // packed column codes of a hot child (3 bytes per non-zero)
    // permuted copy of x behind the packed codes (csr5_hot.hip k_x_permute): table images + frequency-ordered cold regions
    B_COLD_BASE, B_COLD_COLS, B_XPERM,
    // csr5hip_update_values: source map of the slab child (csr5_refresh.hip), 4 bytes per non-zero, built by the first update after
    // a conversion (it depends on the column indices only) and released with the slab structure
    B_REFRESH_MAP,
    SLAB_BUFFERS
};
struct SlabStructure {
    csr5hip_handle_s *child = nullptr;
    int S = 0; // > 0: spmv() runs child + combine
    int m2 = 0;
    int hot_cover_pct = 0;        // share of the non-zeros whose column got a table slot
    int cold_total = 0;           // entries of the cold region
    int sample_stride = 1, min_count = 0; // (hot table) the column sample of the last build (csr5hip_get_slab_view reports them)
    bool values_narrowed = false;
    bool xperm_valid = false;     // (snapshot mode) the copy holds the current x
    bool fallback = false;        // the structure was wanted but could not be built: plain kernel in use
    bool refresh_map_valid = false;
    double t_slab = 0;
    Buffer buf[SLAB_BUFFERS];
    Buffer &operator[](SlabBuf b) { return buf[b]; }
    void release();   // the child and every buffer: the memory goes back
    // asCSR: the slab structure goes out of use but keeps its memory and its child handle, like the arena (capacity only
    // grows until csr5hip_free) -- a reconversion then allocates nothing.  Ten hipMalloc/hipFree pairs were two thirds of
    // the 1.9-ms conversion of a 3 M-nnz matrix.
    void deactivate();
    long long bytes() const; // device memory held: every buffer and the child's conversion arena
};

// ---- transposed companion (csr5hip_build_transpose, csr5_companion.hip): a library-owned CSR of A^T, converted as an ordinary
// handle of shape (n, m) on this handle's stream; released by asCSR / inputCSR / free ----
enum CompanionBuf {
    A_ROW_PTR, A_COL, A_VAL, // the CSR of A^T (col / val in tile order once `at` is converted)
    A_MAP,                   // source map: position in A^T's CSR -> position in A's CSR (4 bytes per non-zero)
    A_STAGE,                 // csr5hip_update_values: the new values in A^T's CSR order
    COMPANION_BUFFERS
};
struct Companion {
    bool built = false; // a companion exists (with nnz = 0: nothing is allocated and `at` stays null)
    csr5hip_handle_s *at = nullptr;
    double t_build = 0; // device build + conversion, ms
    Buffer buf[COMPANION_BUFFERS];
    Buffer &operator[](CompanionBuf b) { return buf[b]; }
    void release();
    long long bytes() const; // the buffers alone: the handle `at` reports its own
};

} // namespace csr5
#pragma GCC visibility pop

struct csr5hip_handle_s {
    int format = -1; // uninitialised until inputCSR, as in the reference
    int value_type = CSR5HIP_F64;
    csr5::Geometry g{};
    int sigma_request = 0; // what setSigma stored (resolved value, >= 1)
    bool sigma_auto = true; // the caller's last sigma request was AUTO (or none): re-resolved for the transposed shape
    int num_offsets = 0;
    hipStream_t stream = nullptr;
    const void *x = nullptr;
    csr5::DeviceArrays d{};
    csr5::SpmvOptions opt{1, 1, 0, 0, 0, 0}; // fused single-launch SpMV, XCD-contiguous tile ranges
    csr5::Requests req;   // what the caller asked for
    bool is_child = false; // internal handle of a slab structure: never builds slabs itself
    bool hot_enabled = false; // (child) its columns are hot-encoded as packed codes next to the plain column words (only the values
                              // are transposed): spmv must use the persistent range kernel
    int xwin_tiles = 0;   // tiles that got a window at conversion
    long long xwin_covered = 0; // non-zeros inside those windows
    long long xwin_lines = 0;   // distinct x lines under the in-window lanes of one sampled gather, summed over those tiles
    // every auxiliary array of the conversion lives in ONE allocation (one hipMalloc, one memset per asCSR5 instead
    // of ten and six: the small-matrix conversion is launch-bound)
    csr5::Buffer b_arena;
    void *scan_tmp = nullptr;
    size_t scan_tmp_bytes = 0;
    uint32_t scalar_words[2] = {0, 0}; // landing zone of the two 4-byte reads of the conversion (checkpoint loading)
    uint32_t *host_words = nullptr;    // 32 pinned, device-visible words the last conversion kernels export into
    // narrow column codes of the x-window kernel (csr5_format.hip k_col16): built when that kernel is selected
    bool col16_built = false;    // the codes of the current conversion exist
    unsigned col16_wide = 0;     // tiles that span >= 32 768 columns (the codes are used only when there is none)
    csr5::Buffer b_col16;        // codes [(p-1) * T / 2 words], then base16 [p]
    // flagged column words of the plain kernel at sigma 4..8 (csr5_format.hip k_col31)
    bool col31_built = false;
    csr5::Buffer b_col31;        // [(p-1) * T words]
    size_t device_total_bytes = 0; // hipMemGetInfo's total, asked once (build_slabs)
    csr5::Buffer b_spmm;         // csr5hip_spmm: carries of one column block, p x spmm_block_width(k) values (first call that needs it)
    double wall_clock_khz = 0;         // rate of the device's constant wall clock (phase stamps)
    double t_malloc = 0, t_tile_ptr = 0, t_tile_desc = 0, t_transpose = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::unordered_map<csr5::GraphKey, hipGraphExec_t, csr5::GraphKeyHash> graphs;
    unsigned generation = 0;    // bumped whenever captured graphs of this handle go stale (csr5hip_spmv_rotate keys on it)
    csr5::SlabStructure slab;
    csr5::Companion comp;

    // csr5hip_spmv_rotate: one graph over several handles (cold-cache measurement protocol)
    hipGraphExec_t rotate_exec = nullptr;
    std::vector<void *> rotate_key;

    size_t vsize() const { return value_type == CSR5HIP_F64 ? 8 : 4; }
    void drop_graphs()
    {
        generation++;
        for (auto &kv : graphs)
            (void)hipGraphExecDestroy(kv.second);
        graphs.clear();
        if (rotate_exec)
            (void)hipGraphExecDestroy(rotate_exec);
        rotate_exec = nullptr;
        rotate_key.clear();
    }
};

#pragma GCC visibility push(hidden)
namespace csr5 {

// ---- csr5_convert.hip: CSR -> CSR5 and back, and the rules that pick the plain path's kernel variant ----
int xwin_decision(const csr5hip_handle_s *h);
int ldsy_decision(const csr5hip_handle_s *h);
int nt_decision(const csr5hip_handle_s *h);
int derive_geometry(csr5hip_handle h, int sigma);
int reserve_aux(csr5hip_handle h);
hipError_t read_format_scalars(csr5hip_handle h, bool sync);
void finish_format_scalars(csr5hip_handle h);
int build_format_arrays(csr5hip_handle h);
int derive_kernel_tables(csr5hip_handle h);
void resolve_variants(csr5hip_handle h);
int prepare_col16(csr5hip_handle h);
int prepare_col31(csr5hip_handle h);
int prepare_plain(csr5hip_handle h);

// ---- csr5_slab_build.hip ----
// The column-slab structure is an optional accelerator: when it cannot be built (allocation failure, memory cap) the
// handle stays a valid CSR5 matrix on the plain tile kernel.  Returns SUCCESS in that case -- csr5hip_info.slab_fallback
// and csr5hip_last_error() say what happened -- unless the caller REQUESTED the structure (req.slab >= 2): then the
// error code is returned (the matrix is still usable on the plain path; csr5hip_as_csr5 additionally rolls back to CSR).
int build_slabs(csr5hip_handle h);
// CSR5HIP_OPT_NARROW_VALUES on the hot child c of h (fp64, nnz > 0): tests its values for fp32 exactness (one synchronisation) and,
// when every one is exact, builds the fp32 copy in h's B_VAL32.  *narrow: the copy exists.  sync_copy: wait for the copy too.
// Touches neither c->d.val32 nor h->slab.values_narrowed: the build fails on an error, the value update falls back.  *copying:
// the error came from building the copy, not from the test.
hipError_t narrow_child_values(csr5hip_handle h, csr5hip_handle c, bool sync_copy, bool *narrow, bool *copying);

} // namespace csr5
#pragma GCC visibility pop
