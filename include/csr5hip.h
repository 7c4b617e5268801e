/*
 * csr5hip.h -- C ABI of libcsr5hip.so: CSR -> CSR5 conversion and CSR5 SpMV on MI355X (gfx950).
 *
 * This is the drop-in boundary for the reference's `anonymouslibHandle<iT, uiT, vT>` class template
 * (CSR5_cuda/anonymouslib_cuda.h:11-53, CSR5_avx2/anonymouslib_avx2.h:11-52).  Every entry point below
 * names the reference member it replaces.  Semantics follow the CUDA variant of the reference: all
 * matrix/vector pointers are DEVICE pointers that the caller allocates, fills and owns; the handle
 * borrows them and allocates only the CSR5 auxiliary arrays (anonymouslib_cuda.h:142-151,188).
 * `include/anonymouslib_hip.h` re-creates the C++ class template on top of this ABI.
 *
 * Fixed instantiation: iT = int32_t, uiT = uint32_t (the only one the reference ever uses,
 * CSR5_cuda/main.cu:59), vT = double or float chosen at create time.  omega = 64 = one wavefront.
 *
 * No torch / HIP types appear in the signatures: streams are passed as `void*` (a hipStream_t).
 */
#ifndef CSR5HIP_H
#define CSR5HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* detail/common.h:13-22 (same numeric values) */
#define CSR5HIP_SUCCESS                   0
#define CSR5HIP_UNKOWN_FORMAT            (-1)
#define CSR5HIP_UNSUPPORTED_CSR5_OMEGA   (-2)
#define CSR5HIP_CSR_TO_CSR5_FAILED       (-3)
#define CSR5HIP_UNSUPPORTED_CSR_SPMV     (-4)
#define CSR5HIP_UNSUPPORTED_VALUE_TYPE   (-5)
/* additions: the reference aborts the process on runtime failures (checkCudaErrors) */
#define CSR5HIP_HIP_ERROR                (-100)
#define CSR5HIP_INVALID_ARGUMENT         (-101)

#define CSR5HIP_FORMAT_CSR   0
#define CSR5HIP_FORMAT_CSR5  1

#define CSR5HIP_OMEGA             64   /* ANONYMOUSLIB_CSR5_OMEGA (detail/cuda/common_cuda.h:11): lanes per tile */
#define CSR5HIP_AUTO_TUNED_SIGMA (-1)  /* ANONYMOUSLIB_AUTO_TUNED_SIGMA (detail/cuda/common_cuda.h:15) */
#define CSR5HIP_MIN_SIGMA          1
#define CSR5HIP_MAX_SIGMA         32   /* the reference instantiates sigma = 4..32 (csr5_spmv_cuda.h:445-540) */

typedef enum { CSR5HIP_F64 = 0, CSR5HIP_F32 = 1 } csr5hip_value_type;

/* csr5hip_set_option keys */
#define CSR5HIP_OPT_SPMV_MODE   1  /* 0 = two-pass (tiles+tail, then calibrate; same summation order as the
                                          reference's three-kernel scheme)
                                      1 = fused single launch [default] (cut rows are finished by the owning
                                          tile or, for long rows, by the last arriving tile; no second launch).
                                      Both modes are bit-reproducible run to run. */
#define CSR5HIP_OPT_XCD_REMAP   2  /* 1 = contiguous tile ranges per XCD (default), 0 = round robin */
#define CSR5HIP_OPT_X_WINDOW    3  /* fused mode: stage a per-tile slice of x in LDS and gather from it.
                                      0 = off, 1 = auto (default: on when the per-tile 4-KB windows of x
                                      chosen at conversion cover >= 70 % of the non-zeros, sigma >= 16 and,
                                      for fp64, a gather spreads over >= 16 lines of x), 2 = force */

#define CSR5HIP_OPT_LDS_Y       4  /* compact a tile's y segments in LDS and flush them with coalesced
                                      stores: 0 = off, 1 = auto (default: on at <= 20 non-zeros per row),
                                      2 = force (applies while 64*sigma*sizeof(vT) <= 8 KiB) */

#define CSR5HIP_OPT_STREAM_NT   5  /* non-temporal loads for the column/value streams: 0 = off, 1 = auto (default: on
                                      when those streams exceed the 256-MiB Infinity Cache, so that a matrix that
                                      cannot stay cached between SpMVs does not evict x either), 2 = force */

#define CSR5HIP_OPT_COLUMN_SLABS 6  /* column-slab structure for matrices whose x exceeds one XCD's L2 and whose columns
                                      are scattered (power-law graphs): the non-zeros are ALSO kept partitioned by a hash
                                      of the column into S slabs, one slab range per XCD, so the eight L2s cache eight
                                      different parts of x; per-(row, slab) partial sums are added in slab order by a small
                                      second kernel (deterministic, no floating-point atomics).  A kernel-side table like
                                      the x-window: the four CSR5 arrays in csr5hip_info are unaffected.
                                      0 = off, 1 = auto (default), 2/4/8/16/32/64 = that many slabs */
#define CSR5HIP_OPT_SLAB_SHIFT  7  /* log2 of the number of adjacent columns hashed to the same slab (default 4 =
                                      one 128-byte line of fp64 x) */
#define CSR5HIP_OPT_SLAB_HOT    9  /* column slabs only: keep each slab's most used columns of x (16 384 fp64 / 32 768 fp32) in a 128-KB
                                      LDS table of a persistent kernel (power-law inputs put most non-zeros on few columns): 0 = off,
                                      1 = auto (default: on when the table covers >= 25 % of the non-zeros), 2 = force */
#define CSR5HIP_OPT_ZERO_EMPTY_ROWS 8 /* 1 = spmv() also stores 0 into rows without non-zeros (so y is fully defined
                                      without the caller zeroing it -- what a solver that feeds y back as x needs);
                                      0 = reference behaviour (default): empty rows before the tail are left untouched */

#define CSR5HIP_OPT_SLAB_MEMORY_MIB 10 /* upper bound, in MiB, on the device memory the column-slab structure may take
                                      (second copy of column_index / value, partial sums, build temporaries); 0 = none
                                      (default).  A structure that would exceed it -- or whose allocation fails -- is
                                      not built: asCSR5() still succeeds and spmv() runs the plain tile kernel
                                      (csr5hip_info.slab_fallback = 1, csr5hip_last_error() says why).  Only a structure
                                      that was REQUESTED (CSR5HIP_OPT_COLUMN_SLABS >= 2) makes asCSR5() fail, after the
                                      matrix has been put back into CSR. */

#define CSR5HIP_OPT_X_SNAPSHOT 11 /* With an LDS hot table the slab kernel gathers from a private, PERMUTED copy of x (every
                                      slab's table image, then its remaining columns in descending order of use: the part of
                                      x a slab reads is dense and its popular prefix stays in one L2).
                                      0 (default) = the copy is taken by every spmv(): x is read live, exactly like the
                                          reference's texture / __ldg gathers (csr5_spmv_cuda.h:7-23) -- a caller may change
                                          x's contents between spmv() calls without telling the handle;
                                      1 = the copy is taken once per setX() (by the first spmv() after it): the caller
                                          promises that x's CONTENTS do not change until the next setX() -- what the
                                          reference CLI does (CSR5_cuda/main.cu:63 "you only need to do it once!", then
                                          NUM_RUN spmv() calls on the same x).  Call setX() again, with the same pointer,
                                          after writing to x.  Handles without a hot table ignore the option. */
#define CSR5HIP_OPT_NARROW_VALUES 12 /* fp64 matrices with an LDS hot table: 1 = when EVERY value of the matrix is exactly
                                      representable as a (normal) fp32 number -- integer weights, 0/1 adjacency, the
                                      reference CLI's rand() % 10 data (CSR5_cuda/main.cu:229-233) -- the slab kernel
                                      streams the values as fp32 and widens them in registers: 4 bytes less per non-zero,
                                      the same products and sums bit for bit (checked on the device at conversion; any
                                      other matrix keeps its fp64 stream).  0 (default) = off: the value stream is the
                                      8-byte one the roofline's algorithmic bytes count.  csr5hip_info.slab_values_narrowed
                                      says what happened.  +4 bytes per non-zero of device memory. */

/* (option numbers 13 and 14 belonged to the range-walking kernel of round 5, which measured slower on every shape and was taken
   out of the product: scripts/experiments/round5/walk_kernel/) */

#define CSR5HIP_OPT_NARROW_COLUMNS 15 /* x-window kernel: when EVERY tile 0 .. p-2 spans fewer than 32 768 columns (banded / blocked
                                      matrices; any matrix with n <= 32 768) the kernel streams 16-bit column codes -- 15 bits of column
                                      minus the tile's smallest column + the element's row-start flag, two per word, kept in a private
                                      array next to column_index -- instead of the 32-bit column words and the descriptor words: 2.25
                                      bytes less per non-zero, the same gathers, bit-identical results.  Built at conversion when a
                                      windowed kernel is selected (sigma 8, 12, 16, 24 or 32); +2 bytes per non-zero of device memory.
                                      1 = auto (default), 0 = off.  csr5hip_info.narrow_columns says what happened. */

#define CSR5HIP_OPT_DEFER_CARRIES 16 /* fused mode, plain path.  A row cut by a tile boundary is normally finished inside the launch: a tile
                                      re-reads a short spill (<= 64 elements) of its last row from the next tile and owns the row, other
                                      cut rows meet in an arrival protocol (one returning atomic per party at the end of its tile).  On
                                      matrices of many tiles both cost more than they save (the spill loads touch sigma cache lines each
                                      in EVERY tile): there no tile finishes a neighbour's spill, every party parks its partial with a
                                      plain store and a second small launch (k_calibrate, the one rows spanning > 64 tiles already use)
                                      adds them in tile order -- the association of the two-pass mode, bit-identical to it; spmv() stays
                                      one call.  1 = auto (default: by tiles, sigma and average row length), 0 = off, 2 = force.
                                      Takes effect at asCSR5(): set it while the matrix is in CSR form.
                                      csr5hip_info.carries_deferred says what happened. */
#define CSR5HIP_OPT_FLAGGED_COLUMNS 18 /* plain fused kernel at sigma 4 .. 8 (short rows: the auto rule's sigma): the kernel streams a private
                                      copy of the tile-ordered column_index that carries the element's row-start flag in bit 31 instead
                                      of column_index + the descriptor words: 256 bytes and one load instruction less per tile, the same
                                      gathers, bit-identical results; the four reference arrays and column_index stay as they are.
                                      +4 bytes per non-zero of device memory.  1 = auto (default: when the column / value streams exceed
                                      the 256-MiB Infinity Cache -- the saving is bytes, not latency: -2.2 % there, +1..5 % on cache-sized
                                      matrices), 0 = off, 2 = force.  csr5hip_info.flagged_columns says what happened. */
/* (option number 17, CSR5HIP_OPT_CARRY_FINISH of round 6 -- the deferred carries added by trailing workgroups of the tile kernel's own
   launch instead of a second launch -- was parity-green and bit-identical but 2 us SLOWER on nd24k-like (the parties' stores must be
   written through to be seen inside the launch) and was taken out again: scripts/experiments/round6/carry_finish_in_launch/) */

typedef struct csr5hip_handle_s *csr5hip_handle;

/* Host-visible snapshot of the handle's private state (anonymouslib_cuda.h:27-52). */
typedef struct csr5hip_info {
    int format;                 /* _format */
    int m, n, nnz;              /* _m, _n, _nnz */
    int value_type;
    int omega;                  /* 64 */
    int sigma;                  /* _csr5_sigma */
    int bit_y_offset;           /* _bit_y_offset */
    int bit_scansum_offset;     /* _bit_scansum_offset */
    int num_packet;             /* _num_packet */
    int p;                      /* _p */
    int tail_partition_start;   /* _tail_partition_start */
    int num_offsets;            /* _num_offsets */
    const uint32_t *d_tile_ptr;    /* _csr5_partition_pointer                  [p+1]                  */
    const uint32_t *d_tile_desc;   /* _csr5_partition_descriptor               [p*omega*num_packet]   */
    const int32_t  *d_offset_ptr;  /* _csr5_partition_descriptor_offset_pointer [p+1]                 */
    const int32_t  *d_offset;      /* _csr5_partition_descriptor_offset        [num_offsets]          */
    int x_window_tiles;            /* tiles that were given an LDS x-window at conversion (ours)      */
    int x_window_active;           /* 1 if spmv() launches the x-window variant                        */
    int x_window_cover_pct;        /* share of the non-zeros (tiles 0..p-2) inside their tile's window */
    int x_window_lines;            /* mean number of distinct 128-B lines of x under the in-window lanes of one gather */
    double t_malloc_ms, t_tile_ptr_ms, t_tile_desc_ms, t_transpose_ms; /* asCSR5 phase timers (:211-214) */
    int column_slabs;              /* S if spmv() runs on the column-slab structure, else 0 (ours)        */
    int slab_shift;                /* log2(columns per hashing granule)                                   */
    int slab_segments;             /* number of (row, slab) segments = rows of the stacked matrix         */
    int slab_sigma, slab_tiles;    /* geometry of the stacked matrix' CSR5 form                           */
    double t_slab_ms;              /* time asCSR5 spent building the slab structure                       */
    int slab_hot;                  /* 1 if the slab kernel gathers hot columns from an LDS table          */
    int slab_hot_cover_pct;        /* share of the non-zeros whose column has a slot in its slab's table  */
    int slab_fallback;             /* 1 = the column-slab structure was wanted but could not be built (memory): the
                                      plain kernel is in use                                                */
    long long device_bytes;        /* device memory held by the handle (CSR5 arrays, kernel tables, slab structure,
                                      build temporaries it keeps); the caller's CSR, x and y are not counted */
    int slab_x_permuted;           /* 1 = the slab kernel gathers from the permuted copy of x (CSR5HIP_OPT_X_SNAPSHOT)   */
    int slab_cold_entries;         /* entries of that copy behind the table images (columns gathered from memory)        */
    int x_snapshot;                /* CSR5HIP_OPT_X_SNAPSHOT as set                                                      */
    int slab_values_narrowed;      /* 1 = CSR5HIP_OPT_NARROW_VALUES took effect: the slab kernel streams fp32 values       */
    int carries_deferred;          /* 1 = cut rows are finished by a second small launch (CSR5HIP_OPT_DEFER_CARRIES)             */
    int narrow_columns;            /* 1 = the x-window kernel streams 16-bit column codes (CSR5HIP_OPT_NARROW_COLUMNS)            */
    int flagged_columns;           /* 1 = the plain kernel streams column words with the row-start flag in bit 31 (CSR5HIP_OPT_FLAGGED_COLUMNS) */
    int lds_y;                     /* 1 = the plain kernel compacts y segments in LDS (CSR5HIP_OPT_LDS_Y and 64*sigma*sizeof(vT) <= 8 KiB) */
    int stream_nt;                 /* 1 = the plain fused kernel streams column_index / value with non-temporal loads (CSR5HIP_OPT_STREAM_NT) */
    int transpose_built;           /* 1 = a transposed companion exists (csr5hip_build_transpose): spmv_t / spmm_t are legal        */
    double t_transpose_build_ms;   /* time csr5hip_build_transpose took: device build of the CSR of A^T + its conversion            */
    int t_sigma, t_p, t_tail_partition_start;          /* the companion's sigma, p, tail_partition_start ...                        */
    int t_column_slabs, t_slab_hot, t_x_window_active; /* ... and the variant its spmv runs (column_slabs, slab_hot, x_window_active) */
} csr5hip_info;

/* anonymouslibHandle(m, n) -- anonymouslib_cuda.h:15.  Uses the current HIP device. */
int csr5hip_create(csr5hip_handle *out, int m, int n, int value_type);
/* Releases the C object (the C++ class has no destructor; callers pair destroy()+scope exit). */
int csr5hip_free(csr5hip_handle h);
/* Stream on which conversion and SpMV are enqueued (the reference uses the default stream). */
int csr5hip_set_stream(csr5hip_handle h, void *hip_stream);

/* warmup() -- anonymouslib_cuda.h:55-59 / format_cuda.h:7-19 */
int csr5hip_warmup(csr5hip_handle h);
/* inputCSR(nnz, row_ptr, col_idx, val) -- anonymouslib_cuda.h:61-76; device pointers, borrowed */
int csr5hip_input_csr(csr5hip_handle h, int nnz, int32_t *d_row_ptr, int32_t *d_col_idx, void *d_val);
/* setX(x) -- anonymouslib_cuda.h:222-260; device pointer, borrowed */
int csr5hip_set_x(csr5hip_handle h, const void *d_x);
/* setSigma(sigma | ANONYMOUSLIB_AUTO_TUNED_SIGMA) -- anonymouslib_cuda.h:294-318 */
int csr5hip_set_sigma(csr5hip_handle h, int sigma);
/* asCSR5() -- anonymouslib_cuda.h:105-220: tile_ptr, tile_desc(+offsets), IN-PLACE tile transpose */
int csr5hip_as_csr5(csr5hip_handle h);
/* asCSR() -- anonymouslib_cuda.h:78-102: inverse transpose, drop the CSR5 arrays */
int csr5hip_as_csr(csr5hip_handle h);
/* spmv(alpha, y) -- anonymouslib_cuda.h:262-284.  Asynchronous on the handle's stream.  As in every
 * reference backend `alpha` is accepted and NOT applied (csr5_spmv_cuda.h:22): y = A*x.
 * Every row that owns a non-zero, and every row >= tail_partition_start, is overwritten; other
 * (empty) rows are left untouched.  Unlike the CUDA variant y need not be zeroed by the caller. */
int csr5hip_spmv(csr5hip_handle h, double alpha, void *d_y);
/* Extension (not in the reference): Y = A*X for k dense vectors.  X: n rows x k, row-major, leading dimension ldx >= k
 * (element (j, c) at X[j*ldx + c]); Y: m rows x k, row-major, ldy >= k.  Device pointers, element-aligned.  Asynchronous on
 * the handle's stream.  Per column c < k, the rows of Y written are spmv()'s (every row that owns a non-zero and every row
 * >= tail_partition_start; the other empty rows only with CSR5HIP_OPT_ZERO_EMPTY_ROWS); columns k .. ldy-1 are never written.
 * Column c is bit-identical to a two-pass spmv() (CSR5HIP_OPT_SPMV_MODE = 0, no column slabs) with x = X[:, c], whatever
 * options the handle carries.  No alpha; the handle's x is neither needed nor touched.  k = 0 is a no-op.  The carry
 * workspace (p tiles x min(8, k rounded up to 1, 2, 4, 8) values) is allocated by the first call that needs it and released by
 * asCSR / destroy / free; later calls with the same k only enqueue work (capturable in a caller's graph).
 * Returns CSR5HIP_INVALID_ARGUMENT for k < 0, ldx < k, ldy < k or null pointers with k > 0, CSR5HIP_UNSUPPORTED_CSR_SPMV
 * in CSR format, CSR5HIP_UNKOWN_FORMAT before inputCSR. */
int csr5hip_spmm(csr5hip_handle h, const void *d_X, int ldx, int k, void *d_Y, int ldy);
/* Extension (not in the reference): replace the matrix' numerical values, keep its pattern and everything derived from it.
 * d_val_csr: nnz values of the handle's value type in CSR order (the order inputCSR's value array had), device pointer,
 * read only, not retained.  It must not overlap the array given to inputCSR.
 * CSR5 format: every later spmv, spmm, spmv_repeat, save and asCSR behaves exactly as if the handle had been built by inputCSR
 * with the new values, the same options and the same sigma, then asCSR5(): bit for bit the same y on every path, the same
 * tile-ordered value array, and asCSR() / destroy() hand the new values back in CSR order.  The conversion is NOT repeated: only
 * the value arrays are rewritten (the handle's own, and with column slabs the stacked matrix' copy and its fp32 image).  The x
 * snapshot (CSR5HIP_OPT_X_SNAPSHOT), the hot table, the permuted x, every column structure, every option and csr5hip_info stay as
 * they are; device_bytes grows only by the helper below.
 * CSR format: a device-to-device copy into the borrowed value array (caller code need not know the format).
 * Asynchronous on the handle's stream: ordered after earlier spmv() calls and before later ones; d_val_csr must stay valid and
 * unchanged until the work has run.  With column slabs the FIRST call after a conversion allocates and builds a pattern-only
 * helper (4 bytes per non-zero: where every element of the stacked matrix comes from; one host synchronisation; counted in
 * device_bytes; released with the slab structure); later calls only enqueue work, so update_values + spmv can be captured in a
 * caller's graph on one stream.  One exception: a hot-table handle with CSR5HIP_OPT_NARROW_VALUES = 1 re-checks on every call
 * that each new value is an exact fp32 number, which takes one host synchronisation (such a call cannot be captured);
 * csr5hip_info.slab_values_narrowed reports the outcome.  When that outcome changes the library drops its own graphs
 * (spmv_repeat / spmv_rotate re-record), and a graph the CALLER captured from this handle must be captured again.
 * Returns CSR5HIP_INVALID_ARGUMENT for a null handle, a null pointer with nnz > 0 or a pointer that overlaps the handle's own
 * value array; CSR5HIP_UNKOWN_FORMAT before inputCSR; CSR5HIP_HIP_ERROR (see csr5hip_last_error) when the helper cannot be
 * allocated or the call cannot be captured -- the handle is then unchanged and still usable.  nnz = 0 is a successful no-op. */
int csr5hip_update_values(csr5hip_handle h, const void *d_val_csr);
/* Extension (not in the reference): products with the transpose, y = A^T x, on the converted handle.
 * csr5hip_build_transpose gives a handle in CSR5 format a TRANSPOSED COMPANION: a library-owned CSR of A^T (n rows, m columns)
 * built on the device from the handle's tile-ordered arrays, then converted to CSR5 as an ordinary internal handle on the same
 * stream.  Row j of A^T holds A's entries of column j in ascending order of their position in A's CSR arrays (ascending row;
 * repeated (row, column) pairs keep the order they have in A) -- what a stable sort of the CSR column array gives -- so every
 * result equals, bit for bit, that of a handle the caller builds by hand from such a transposed CSR with the same value type,
 * sigma request and options.  The companion carries the sigma request last made on this handle (AUTO is re-resolved for the
 * transposed shape, csr5hip_auto_sigma(n, nnz, type)) and every csr5hip_set_option value of this handle, at build time and
 * whenever one is set later, except CSR5HIP_OPT_X_SNAPSHOT (0: spmv_t reads its x live).  A column-slab structure that only
 * the auto rule wanted and that does not fit CSR5HIP_OPT_SLAB_MEMORY_MIB falls back as on any handle.
 * The call allocates and synchronises (not capturable: CSR5HIP_HIP_ERROR + csr5hip_last_error while the stream is capturing).
 * A no-op when a companion exists; with nnz = 0 it succeeds and allocates nothing.  The handle's own arrays, results, graphs
 * and csr5hip_info (apart from the fields below and device_bytes) are untouched.  If anything fails, everything allocated for
 * the companion is released, the handle stays usable and the error is returned.
 * Memory (csr5hip_info.device_bytes counts all of it): the CSR of A^T (nnz x (4 + sizeof value) + 4 (n + 1) bytes), its CSR5
 * arrays and kernel tables, the source map (4 bytes per non-zero: position in A^T's CSR -> position in A's) and a staging
 * buffer of nnz values for csr5hip_update_values.
 * Lifetime: released by asCSR / destroy / free and inputCSR (csr5hip_autotune_sigma re-converts and so drops it); save / load
 * do not carry it, a loaded handle can build one.  csr5hip_update_values on this handle also gives the companion the new
 * values, on the same stream behind the handle's own update (with column slabs on the companion its first such call builds
 * that structure's helper and synchronises once; later calls only enqueue).
 * Returns CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format, CSR5HIP_UNKOWN_FORMAT before inputCSR.
 * Single handles only: csr5hip_multi has no transposed product (A^T of a row block needs a sum across the shards). */
int csr5hip_build_transpose(csr5hip_handle h);
/* y = A^T x.  d_x: m values, d_y: n values, device pointers.  Asynchronous on the handle's stream, enqueue-only (capturable in
 * a caller's graph on that stream).  The handle's own x (setX) is neither needed nor touched; no alpha.  Rows of y follow
 * spmv()'s contract on the transposed matrix: every row of A^T that owns a non-zero and every row >=
 * csr5hip_info.t_tail_partition_start is overwritten, other empty rows only with CSR5HIP_OPT_ZERO_EMPTY_ROWS.
 * Returns CSR5HIP_INVALID_ARGUMENT for null pointers or when no companion exists (csr5hip_last_error: call
 * csr5hip_build_transpose first -- it is never built lazily), CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format,
 * CSR5HIP_UNKOWN_FORMAT before inputCSR. */
int csr5hip_spmv_t(csr5hip_handle h, const void *d_x, void *d_y);
/* Y = A^T X for k dense vectors: csr5hip_spmm's contract on the companion (X: m rows x k, ldx >= k; Y: n rows x k, ldy >= k;
 * column c bit-identical to a two-pass spmv of the transposed matrix with x = X[:, c]); errors as csr5hip_spmm and
 * csr5hip_spmv_t. */
int csr5hip_spmm_t(csr5hip_handle h, const void *d_X, int ldx, int k, void *d_Y, int ldy);
/* Extension (not in the reference): sampled dense-dense product on the matrix' own pattern,
 *     out[e] = sum_{c < k} U[row(e), c] * V[col(e), c]      for every stored element e of A.
 * U: m rows x k, row-major, leading dimension ldu >= k; V: n rows x k, row-major, ldv >= k; d_out_csr: nnz values of the handle's
 * value type in CSR ORDER -- the order inputCSR's value array had and csr5hip_update_values takes (repeated (row, column) pairs
 * each get their own, equal, output).  Device pointers, element-aligned.  With U = dY and V = X this is the gradient of
 * Y = A X with respect to A's stored values; csr5hip_spmm_t gives the one for X.
 * The matrix VALUES play no part: the pattern samples, the values do not scale.  The handle's x, its values, every option,
 * csr5hip_info and device_bytes are neither read nor changed; nothing is allocated: the call only enqueues work on the handle's
 * stream, from the first call on (capturable in a caller's graph on that stream).  Rows and columns come from the handle's own
 * tile structure (tile_ptr, the bit flags, y_offset, the empty-row offsets, the tile-ordered column_index), whatever path spmv()
 * runs on the handle.
 * DETERMINISM: out[e] is ONE chain of k fused multiply-adds in ascending column order onto +0,
 *     fma(U[r][k-1], V[j][k-1], ... fma(U[r][1], V[j][1], fma(U[r][0], V[j][0], +0)) ...),
 * so it depends only on the k values of U's row, the k values of V's row, k and the value type: not on sigma, any option, the
 * element's position or the kind of tile that holds it, ldu / ldv, pointer alignment or the run.  A dot product is computed
 * from its own two rows only (Inf and NaN stay with the elements whose rows hold them); subnormals are not flushed.
 * k = 0 writes +0 into all nnz outputs; nnz = 0 is a successful no-op.  d_out_csr must not overlap U, V or any array of the
 * handle (the CSR arrays given to inputCSR included); U and V may be the same array.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, k < 0, ldu < k, ldv < k, a null U or V with k > 0 and
 * nnz > 0, or a null d_out_csr with nnz > 0; CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format; CSR5HIP_UNKOWN_FORMAT before inputCSR.
 * Single handles only: csr5hip_multi has no sddmm (a shard holds a row block: call it on the shard handles with U's row block). */
int csr5hip_sddmm(csr5hip_handle h, const void *d_U, int ldu, const void *d_V, int ldv, int k, void *d_out_csr);
/* Extension (not in the reference): softmax over the stored entries of every row ("edge softmax") and its gradient, on arrays of
 * nnz values of the handle's value type in CSR ORDER (the order inputCSR's value array had, csr5hip_sddmm writes and
 * csr5hip_update_values takes):
 *     csr5hip_row_softmax        out[e] = exp(s[e] - M_r) / Z_r,   M_r = max of the row's scores, Z_r = sum_row exp(s[j] - M_r)
 *     csr5hip_row_softmax_grad   out[e] = p[e] * (g[e] - D_r),     D_r = sum_row p[j] * g[j]   (p: the forward's output,
 *                                                                   g: the gradient arriving for it)
 * Device pointers, element-aligned.  d_out_csr must not overlap an input or any array of the handle; d_p_csr and d_g_csr may be
 * the same array.  Both read the handle's row_ptr and NOTHING else (no columns, values, x, tile structure or kernel table), so
 * they are legal in CSR and in CSR5 format alike.  Nothing is allocated and nothing in the handle changes (csr5hip_info,
 * device_bytes, the values, x and the options stay as they are); the call only enqueues work on the handle's stream, from the
 * first call on (capturable in a caller's graph on that stream; no pre-pass, nothing read back).
 * DEFINITION: M is the exact maximum of the row; a term is one subtraction and one exponential (the device library's full
 * precision exp / expf, subnormal results kept); the quotient is ONE RECIPROCAL PER ROW, r = 1 / Z (correctly rounded), and ONE
 * MULTIPLICATION PER ENTRY.  The gradient rounds each p[j] * g[j], then g[e] - D, then the product with p[e]; no fused
 * multiply-add, no rescaled running maximum.  D is computed from the row's own entries only.
 * Empty rows write nothing; a finite row of one entry gives exactly 1.  NON-FINITE values follow torch.softmax: a -Inf score gets
 * exactly +0; a row that holds a NaN, holds a +Inf or consists only of -Inf gives NaN in every entry of that row and in no other.
 * TREE of Z and of D, a function of the row's length L alone.  L <= 512: slot(j) = j mod 64; every slot adds its terms j = slot,
 * slot + 64, ... in ascending order onto +0; the 64 slot sums (+0 where a slot has no term) are added by the balanced binary tree
 * over adjacent slots (pairs (0,1) (2,3) ..., quads, ..., the two halves).  L > 512: slot(j) = j mod 256, slots 64 w .. 64 w + 63
 * by that balanced tree for w = 0 .. 3, then (w0 + w1) + (w2 + w3).
 * DETERMINISM: the bits of a row's outputs depend only on that row's inputs (values and order) and on the value type: not on
 * sigma, any option or the format, pointer alignment, m, nnz, the position of the row in the matrix, what neighbouring rows
 * hold, or the run.
 * A row is worked on by at most one workgroup (rows beyond 512 entries by its four wavefronts together), so one very long row
 * runs at one workgroup's bandwidth.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle or any null pointer while nnz > 0;
 * CSR5HIP_UNKOWN_FORMAT before inputCSR.  nnz = 0 is a successful no-op that touches no device.
 * Single handles only: csr5hip_multi has none (a shard holds whole rows: call them on the shard handles). */
int csr5hip_row_softmax(csr5hip_handle h, const void *d_scores_csr, void *d_out_csr);
int csr5hip_row_softmax_grad(csr5hip_handle h, const void *d_p_csr, const void *d_g_csr, void *d_out_csr);
/* Extension (not in the reference): attention on the matrix' own pattern in ONE pass -- scores, softmax over the row, product:
 *     s_e     = sum_{c < k} Q[i, c] * K[j_e, c]          for the stored entries e of row i in CSR order, j_e the column of e
 *     O[i, c] = (sum_e exp(s_e - M_i) * V[j_e, c]) / Z_i,   M_i = max_e s_e,  Z_i = sum_e exp(s_e - M_i),   c < d
 * i.e. what csr5hip_sddmm -> csr5hip_row_softmax -> csr5hip_update_values -> csr5hip_spmm compute, without anything of length nnz
 * written to memory and without touching the handle: its values, x, options, csr5hip_info and device_bytes are neither read nor
 * changed (the matrix VALUES play no part), nothing is allocated, nothing is read back.  The call only enqueues one kernel on the
 * handle's stream, from the first call on (capturable in a caller's graph on that stream).
 * Q: m x k (ldq >= k), K: n x k (ldk >= k), V: n x d (ldv >= d), O: m x d (ldo >= d); all row-major, device pointers,
 * element-aligned, of the handle's value type.  Column slices of wider tensors are legal operands (one call per head on
 * Q[:, h k .. (h + 1) k) with ldq = H k needs no copy).  O must not overlap Q, K, V or any array of the handle; Q, K and V may be
 * the same array.  Repeated (row, column) pairs are separate entries.
 * EVERY row of O is written in columns 0 .. d-1: a row without entries gets +0 -- unlike csr5hip_spmm, which leaves such rows
 * alone -- so O may be uninitialised memory.  Columns d .. ldo-1 are never written.
 * k = 0 makes every score +0: each output is the mean of the row's V rows.  d = 0 or m = 0 is a successful no-op; nnz = 0 with
 * d > 0 writes the zeros.
 * DEFINITION: s_e is csr5hip_sddmm's chain of k fused multiply-adds in ascending column order onto +0, the same bits; M is the
 * exact maximum of the row; a weight w_e = exp(s_e - M) is ONE subtraction and ONE exponential (the device library's full
 * precision exp / expf, subnormal results kept).  THE NORMALISATION COMES AFTER THE PRODUCT: acc_c = sum_e w_e V[j_e, c] by fused
 * multiply-adds, ONE reciprocal per row r = 1 / Z (correctly rounded) and ONE multiplication per output, O[i, c] = acc_c * r.  No
 * running maximum is rescaled.
 * NON-FINITE values behave as the unfused chain: a -Inf score has weight +0; a row that holds a NaN score, holds a +Inf score or
 * consists only of -Inf scores is NaN in all d outputs, and no other row is affected.
 * SUMMATION ORDER, a function of (L, d) alone, L the row's length and j an entry's rank inside its row.
 *   Z:  csr5hip_row_softmax's tree.  L <= 512: slot(j) = j mod 64, every slot adds its terms in ascending order onto +0, the 64
 *       slot sums (+0 where a slot has no term) by the balanced binary tree over adjacent slots.  L > 512: slot(j) = j mod 256,
 *       slots 64 w .. 64 w + 63 by that tree for w = 0 .. 3, then (w0 + w1) + (w2 + w3).
 *   acc_c, L <= 16: one chain acc = fma(w_j, V[j_j, c], acc) over j = 0 .. L-1 onto +0.
 *   acc_c, L > 16:  column c lies in block b = c / 64 of width wb = min(64, d - 64 b); C = the smallest power of two >= wb;
 *       S = 64 / C slots for L <= 512 and 256 / C for L > 512; slot(j) = j mod S; every slot runs one such chain over its j in
 *       ascending order onto +0; the S slot sums (+0 where a slot has no term) by the balanced binary tree over adjacent slots.
 * DETERMINISM: the bits of row i of O depend only on Q's row i, the K and V rows of the row's columns in their CSR order, k, d
 * and the value type: not on sigma, any option, the kind of tile that holds the row's entries, the row's position, its
 * neighbours, m, n, nnz, the leading dimensions, pointer alignment or the run.
 * A row is worked on by at most one workgroup (rows up to 16 entries by 16 lanes, up to 512 by one wavefront, longer ones by the
 * four wavefronts together; beyond 2 048 entries the scores are computed twice), so one very long row runs at one workgroup's
 * rate.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, k < 0, d < 0, ldq < k, ldk < k, ldv < d,
 * ldo < d, a null Q or K with k > 0 and nnz > 0, a null V with d > 0 and nnz > 0, or a null O with d > 0 and m > 0;
 * CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format; CSR5HIP_UNKOWN_FORMAT before inputCSR.
 * Single handles only: csr5hip_multi has no such call (a shard holds whole rows: call it on the shard handles). */
int csr5hip_attention(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                      const void *d_V, int ldv, int d, void *d_O, int ldo);
/* Extension (not in the reference): the gradients of csr5hip_attention's O for Q, K and V in TWO launches, with nothing of length nnz
 * written and the handle untouched.  d_dO is the gradient arriving for O (m x d, lddo >= d).  Per stored entry e = (i, j):
 *     p_e  = exp(s_e - M_i) * r_i   (s_e, M_i, Z_i as in csr5hip_attention, r_i = 1 / Z_i: csr5hip_row_softmax's bits)
 *     dp_e = sum_{c < d} dO[i, c] * V[j, c]   (csr5hip_sddmm's chain: d fused multiply-adds in ascending column order onto +0)
 *     D_i  = sum over row i of round(p_e * dp_e) by Z's tree,   ds_e = p_e * (dp_e - D_i)   (csr5hip_row_softmax_grad's bits)
 *     dQ[i, c] = sum_e ds_e K[j_e, c]  (m x k)    dK[j, c] = sum_e ds_e Q[i_e, c]  (n x k)    dV[j, c] = sum_e p_e dO[i_e, c]  (n x d)
 * ANY OUTPUT MAY BE NULL: it is not wanted; with all three null the call is a successful no-op.  EVERY row of a wanted output is
 * written in its k (d) columns -- a row or column of the matrix without entries gets +0 -- and nothing beyond them, so the outputs
 * may be uninitialised memory.  Outputs must not overlap the inputs, each other, the workspace or any array of the handle.
 * d_work: caller-owned scratch of 4 * m values of the handle's type (layout private: per row M, r, D and one unused value); needed
 * only when dK or dV is wanted.  dK or dV REQUIRES THE TRANSPOSED COMPANION (csr5hip_build_transpose; never built lazily): the row
 * kernel walks the parent's pattern, writes dQ and the workspace; the column kernel walks the companion's pattern, gathers the
 * workspace values of every entry's row, recomputes s_e and dp_e and writes dK and dV.  dQ alone needs neither.
 * The call allocates nothing, reads nothing back, only enqueues on the handle's stream from the first call on (capturable), and
 * neither reads nor changes the handle's values, x, options, csr5hip_info or device_bytes.
 * SUMMATION ORDER: every accumulation is csr5hip_attention's acc_c rule as a function of (L, width) alone: dQ with (row length, k),
 * dK with (column length, k), dV with (column length, d); a column's entries are taken in A's CSR order.  DETERMINISM: the bits of
 * a row of dQ depend only on that row's operands, those of a row of dK or dV only on its column's entries and those rows'
 * operands: not on sigma (the parent's or the companion's), any option, leading dimensions, pointer alignment or the run.
 * NON-FINITE: a row whose forward output is NaN gives NaN in its dQ row and in the dK and dV rows of exactly the columns it stores;
 * every other output row is unaffected; a -Inf score has p = +0.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, k < 0, d < 0 or a leading dimension below
 * its width (ldq, ldk, lddq, lddk < k; ldv, lddo, lddv < d); CSR5HIP_INVALID_ARGUMENT, when an output is wanted and nnz > 0, for a
 * null Q or K with k > 0, a null V or dO with d > 0, or a null workspace with dK or dV wanted; CSR5HIP_INVALID_ARGUMENT with a
 * csr5hip_last_error text when dK or dV is wanted and there is no companion; CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format;
 * CSR5HIP_UNKOWN_FORMAT before inputCSR.  nnz = 0 only writes the zeros.  Single handles only. */
int csr5hip_attention_backward(csr5hip_handle h, const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                               const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                               void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work);
/* Extension (not in the reference): csr5hip_attention for `heads` heads in ONE launch, on PACKED operands: head h (0 <= h < heads)
 * reads Q[:, h k .. h k + k) and K[:, h k .. h k + k), reads V[:, h d .. h d + d) and writes O[:, h d .. h d + d).  Rows are
 * row-major with ldq, ldk >= heads * k and ldv, ldo >= heads * d (the layout (rows, heads, width) of every framework); the operands
 * may themselves be column slices of wider tensors.
 * DEFINITION BY REFERENCE: head h of O is, bit for bit, what
 *     csr5hip_attention(h, Q + h k, ldq, K + h k, ldk, k, V + h d, ldv, d, O + h d, ldo)
 * writes -- for every row class, for non-finite scores, for rows without entries (+0) and for k = 0 -- so the summation orders, the
 * score chain, the one reciprocal per row and the determinism contract are that call's.  One rule differs: 16-byte loads are taken
 * only where every head's slice of every row is 16-byte aligned, i.e. under that call's conditions and (k * sizeof) % 16 == 0;
 * either load width feeds the same chains.  heads = 1 IS csr5hip_attention.
 * What is done once for all heads: a row's bounds and class, an entry's rank -> storage map and its column load; per entry the
 * heads are taken one after the other.  The heads may be split into contiguous groups over the grid's second dimension; the
 * number of groups is a function of (m, heads) alone and no bit depends on it.
 * As csr5hip_attention: nothing is allocated or read back, the call only enqueues one kernel on the handle's stream from the first
 * call on (capturable), and the handle's values, x, options, csr5hip_info and device_bytes are neither read nor changed.  EVERY row
 * of O is written in all heads * d columns; columns heads * d .. ldo-1 are never written.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0, ldq or ldk
 * < heads * k, ldv or ldo < heads * d (compared in 64 bits), and with heads > 0 for the null operands csr5hip_attention rejects;
 * CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format; CSR5HIP_UNKOWN_FORMAT before inputCSR.  heads = 0, like d = 0 or m = 0, is then a
 * successful no-op.  Single handles only. */
int csr5hip_mha(csr5hip_handle h, int heads,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo);
/* Extension (not in the reference): csr5hip_attention_backward for `heads` heads in TWO launches, on csr5hip_mha's packed layout:
 * dO and dV as V (head h in columns h d .. h d + d), dQ and dK as Q (columns h k .. h k + k); lddo, lddv >= heads * d and lddq,
 * lddk >= heads * k.  Head h of every wanted output is, bit for bit, what csr5hip_attention_backward on the same slices writes;
 * 16-byte loads only where additionally (k * sizeof) % 16 == 0 and (d * sizeof) % 16 == 0.  Any output may be null; every row of a
 * wanted one is written in all its heads * k (heads * d) columns and nothing beyond.
 * d_work: caller-owned scratch of 4 * m * heads values of the handle's type (layout private; the heads of a row are adjacent),
 * needed only when dK or dV is wanted.  dK or dV REQUIRES THE TRANSPOSED COMPANION (csr5hip_build_transpose; never built lazily).
 * The head groups of the row kernel are a function of (m, heads), those of the column kernel of (n, heads).
 * Allocates nothing, reads nothing back, only enqueues (capturable), leaves the handle untouched.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0 or a leading dimension below heads
 * times its width (64-bit comparison); CSR5HIP_INVALID_ARGUMENT, with heads > 0, for the null operands csr5hip_attention_backward
 * rejects; CSR5HIP_INVALID_ARGUMENT with a csr5hip_last_error text when dK or dV is wanted and there is no companion;
 * CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format; CSR5HIP_UNKOWN_FORMAT before inputCSR.  heads = 0 is then a successful no-op. */
int csr5hip_mha_backward(csr5hip_handle h, int heads,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work);
/* Extension (not in the reference): csr5hip_mha_biased and csr5hip_mha_biased_backward -- csr5hip_mha / csr5hip_mha_backward with a
 * softmax scale and an additive score bias taken from the handle's stored values -- are declared, with their contracts, in
 * csr5hip_bias.h, which this header includes at its end.  (A file of its own because tests/test_host.py compares the names declared
 * in THIS file's text with the Python binding's main symbol list, which tests/test_mha_host.py in turn pins for the csr5hip_mha
 * prefix; the two calls' declarations and exports are compared by tests/test_mha_bias_host.py.) */
/* Extension (not in the reference): csr5hip_mha_edge_bias and csr5hip_mha_edge_bias_backward -- csr5hip_mha / csr5hip_mha_backward with
 * a softmax scale and a per-head additive score bias taken from a caller-owned (nnz, heads) tensor in CSR order, the handle's values
 * left unread -- are declared, with their contracts, in csr5hip_edge_bias.h, which this header includes at its end for the same
 * reason; their declarations and exports are compared by tests/test_mha_edge_bias_host.py. */
/* Extension (not in the reference): csr5hip_mha_lowp -- csr5hip_mha_edge_bias on operands stored in bf16 or fp16, computed in fp32
 * and rounded once -- is declared, with its contract and its operand-type constants, in csr5hip_lowp.h, which this header includes at
 * its end for the same reason; its declaration and export are compared by tests/test_mha_lowp_host.py. */
/* Extension (not in the reference): csr5hip_gat and csr5hip_gat_backward -- additive (GAT, GATv2) attention, whose score
 * fma(sum_c a_c LeakyReLU(q_c + k_c), scale, B) no choice of Q, K and B turns into a dot product -- are declared, with their contracts,
 * in csr5hip_gat.h, which this header includes at its end for the same reason; their declarations and exports are compared by
 * tests/test_gat_host.py. */
/* Extension (not in the reference): csr5hip_dropout_mha, csr5hip_dropout_gat, their backwards and csr5hip_dropout_mask -- the edge-bias
 * and the additive call with a seeded dropout mask on the attention weights, recomputed in the backward, and the mask itself -- are
 * declared, with their contracts and the mask's definition, in csr5hip_dropout.h, which this header includes at its end for the same
 * reason; their declarations and exports are compared by tests/test_attention_dropout_host.py. */
/* Extension (not in the reference): csr5hip_dropout_mha_lowp and csr5hip_dropout_mha_lowp_backward -- the dropped dot-product calls on
 * operands stored in bf16 or fp16, computed in fp32 and rounded once -- are declared, with their contracts, in csr5hip_dropout_lowp.h,
 * which this header includes at its end for the same reason; their declarations and exports are compared by
 * tests/test_dropout_lowp_host.py. */
/* `count` back-to-back spmv() calls replayed from one captured hipGraph (the reference CLI's timed
 * loop, CSR5_cuda/main.cu:96-99, without per-launch host cost). */
int csr5hip_spmv_repeat(csr5hip_handle h, double alpha, void *d_y, int count);
/* Cold-cache measurement protocol: `count` SpMVs replayed from ONE hipGraph on hs[0]'s stream, the i-th using handle
 * hs[i % k] and the vector d_ys[i % k].  With k copies of a matrix (each with its own x and y) whose total footprint
 * exceeds the 256-MiB Infinity Cache, every SpMV streams its operands from HBM instead of finding them cached from
 * the previous launch (the reference's timed loop, CSR5_cuda/main.cu:96-99, re-reads one matrix). */
int csr5hip_spmv_rotate(csr5hip_handle *hs, void **d_ys, int k, double alpha, int count);
/* CSR5HIP_OPT_X_SNAPSHOT = 1 only: take the permuted copy of x NOW, on the handle's stream, instead of in front of the first
 * spmv() after setX (so that no spmv() of a timed loop carries it).  A no-op for handles without a hot table, in live-x mode,
 * before asCSR5 / setX, or when the copy is current. */
int csr5hip_snapshot_x(csr5hip_handle h);
/* destroy() -- anonymouslib_cuda.h:286-291 (== asCSR) */
int csr5hip_destroy(csr5hip_handle h);

/* Measured sigma selection (what ANONYMOUSLIB_AUTO_TUNED_SIGMA's per-architecture tables approximate,
 * anonymouslib_cuda.h:297-313): converts with each candidate sigma, times a hipGraph batch of SpMVs into
 * d_y and leaves the matrix in CSR5 with the fastest one.  Call after inputCSR + setX; d_y is overwritten. */
int csr5hip_autotune_sigma(csr5hip_handle h, void *d_y, int *best_sigma, double *best_us);

int csr5hip_set_option(csr5hip_handle h, int option, int value);
int csr5hip_get_info(csr5hip_handle h, csr5hip_info *info);

/* Read-only view of the column-slab child WITH an LDS hot table (csr5hip_info.slab_hot == 1), for tests and inspection: what the
 * conversion decided, array by array.  Scalars, and device pointers that are BORROWED from the handle: they stay valid until the
 * next conversion (asCSR5, asCSR, inputCSR), the next csr5hip_set_option or csr5hip_free on this handle; copy them out with
 * csr5hip_memcpy_d2h.  xperm holds the last x that spmv() (or csr5hip_snapshot_x) permuted.  A struct of its own: csr5hip_info's
 * layout is mirrored by callers and does not grow for this. */
typedef struct csr5hip_slab_view {
    int S;                   /* slabs                                                                                   */
    int capacity;            /* table slots per slab (slot 0 is reserved)                                               */
    int slab_shift, slab_bits; /* slab of a column = xor of all slab_bits-wide groups of (column >> slab_shift)         */
    int sigma, T, p;         /* the child's sigma, tile elements (64 sigma) and tiles (tile p - 1 is the CSR tail)      */
    int tail_start;          /* first child row of the CSR tail                                                         */
    int segments;            /* rows of the child = (row, slab) segments                                                */
    int cold_total;          /* entries of the cold region                                                              */
    int stride, min_count;   /* the column sample: one 64-element chunk in `stride`; uses a column needs for a slot     */
    int values_narrowed;     /* 1 = val32 is in use (CSR5HIP_OPT_NARROW_VALUES)                                         */
    const int32_t *slab_off;    /* [S + 1] first child element of every slab                                            */
    const int32_t *hot_tile0;   /* [S + 1] first tile owned by every slab, then [S] the slabs of XCD 0, 1, ...           */
    const int32_t *hot_count;   /* [S] slots in use, the reserved slot 0 included                                        */
    const int32_t *hot_cols;    /* [S * capacity] column of every slot                                                   */
    const int32_t *cold_base;   /* [S + 1] start of every slab's cold entries                                            */
    const int32_t *cold_cols;   /* [cold_total] column of every cold entry                                               */
    const uint16_t *col_lo;     /* low 16 bits of the packed column codes, child CSR order, tiles 0 .. p-2               */
    const uint8_t *col_hi;      /* their high 8 bits: 0x80 = table slot, 0x40 = the element starts a child row           */
    const int32_t *row_ptr;     /* [segments + 1] the child's row pointer                                                */
    const int32_t *col;         /* [nnz] its plain column indices, CSR order                                             */
    const void *val;            /* [nnz] its values: tiles 0 .. p-2 in lane-major 16-byte pieces, the tail in CSR order  */
    const float *val32;         /* the same as fp32 in pieces of four (values_narrowed), else NULL                       */
    const uint32_t *tile_ptr;   /* [p + 1]                                                                               */
    const int32_t *range_begin; /* [S * 257] first tile of every wavefront range of every slab                           */
    const unsigned long long *range_cost; /* [p] prefix costs of tiles 0 .. p-2 (entry 0 is 0), the cuts' input          */
    const uint32_t *range_head; /* [S * 256 + 1] first child row of every range | 0x80000000, then the CSR tail's        */
    const void *xperm;          /* [S * capacity] table images of x, then [cold_total] its cold region                   */
} csr5hip_slab_view;
/* Fills *out.  Launches nothing and allocates nothing.  Returns CSR5HIP_INVALID_ARGUMENT, with a csr5hip_last_error text and *out
 * untouched, for null arguments and for a handle without a hot slab child: not converted, no column slabs, or
 * csr5hip_info.slab_hot == 0. */
int csr5hip_get_slab_view(csr5hip_handle h, csr5hip_slab_view *out);

/* sigma that setSigma(AUTO) would pick for (m, nnz, value_type) on gfx950 */
int csr5hip_auto_sigma(int m, int nnz, int value_type);
const char *csr5hip_last_error(void);
const char *csr5hip_version(void);

/* ---- device shims so that a plain g++ host program (the ./spmv CLI, CSR5_cuda/main.cu:17-117) can
 *      allocate and move the caller-owned arrays without including HIP headers ---- */
int csr5hip_device_count(int *count);
int csr5hip_set_device(int device);
int csr5hip_device_name(int device, char *buf, size_t buflen, double *clock_mhz);
int csr5hip_malloc(void **dptr, size_t bytes);
int csr5hip_device_free(void *dptr);
int csr5hip_memcpy_h2d(void *dst, const void *src, size_t bytes);
int csr5hip_memcpy_d2h(void *dst, const void *src, size_t bytes);
int csr5hip_memset(void *dptr, int value, size_t bytes);
int csr5hip_synchronize(void);
/* event pair on the handle's stream: elapsed device time in ms between the two calls */
int csr5hip_timer_start(csr5hip_handle h);
int csr5hip_timer_stop(csr5hip_handle h, double *ms);

/* ---------------------------------------------------------------------------------------------------
 * Matrix Market ingest and COO -> CSR: the step BEFORE the path.
 * Replaces the serial fscanf loop and the host counting scatter of the reference CLI
 * (CSR5_avx2/main.cpp:126-281, CSR5_cuda/main.cu reads through the same code) with a multi-threaded
 * mmap parser and a device-side stable sort; the resulting CSR is identical, entry for entry, to the
 * one the reference builds (file order inside a row; the mirror of a symmetric off-diagonal follows
 * its original).
 * ------------------------------------------------------------------------------------------------- */
#define CSR5HIP_MTX_CANNOT_OPEN   (-1)   /* CLI exit codes, main.cpp:135-157 */
#define CSR5HIP_MTX_BAD_BANNER    (-2)
#define CSR5HIP_MTX_COMPLEX       (-3)
#define CSR5HIP_MTX_BAD_SIZE      (-4)   /* also: fewer entries in the file than the size line announces */

#define CSR5HIP_FIELD_REAL     0
#define CSR5HIP_FIELD_INTEGER  1
#define CSR5HIP_FIELD_PATTERN  2

/* COO triplets of a .mtx file: 0-based, file order, host memory owned by the library. */
typedef struct csr5hip_mtx {
    int32_t m, n;
    int64_t nz;            /* entries in the file (nnzA_mtx_report, main.cpp:132) */
    int field;             /* CSR5HIP_FIELD_* ; pattern entries get the value 1.0 (main.cpp:198) */
    int symmetric;         /* 1 for a symmetric or hermitian banner (main.cpp:159-163); skew-symmetric is NOT expanded */
    int32_t *row, *col;    /* [nz] */
    double *val;           /* [nz] */
    int threads;           /* parser threads used */
    int fast_path;         /* 1 = parallel line parser, 0 = sequential fscanf-compatible scanner */
    double t_parse_ms;
    int64_t file_bytes;
    int alloc_flags;       /* reserved (0) */
} csr5hip_mtx;

/* Device CSR built from COO; every d_* array is allocated here, release with csr5hip_csr_release. */
typedef struct csr5hip_csr {
    int32_t m, n, nnz;
    int32_t *d_row_ptr;    /* [m+1] */
    int32_t *d_col_idx;    /* [nnz] */
    void *d_val;           /* [nnz] of value_type, or NULL when no values were requested */
    int value_type;
    double t_parse_ms, t_h2d_ms, t_build_ms;   /* filled by csr5hip_mtx_load / csr5hip_coo_to_csr */
} csr5hip_csr;

/* Parse `path` (threads <= 0: one per hardware thread, capped at 64).  Returns 0 or CSR5HIP_MTX_*;
 * CSR5HIP_INVALID_ARGUMENT for an index outside [1,m] x [1,n] (the reference would corrupt memory). */
int csr5hip_mtx_read(const char *path, int threads, csr5hip_mtx *out);
int csr5hip_mtx_release(csr5hip_mtx *mtx);

/* main.cpp:213-275 on the device.  d_row / d_col / d_val: nz COO triplets in file order (d_val may be
 * NULL: structure only, out->d_val = NULL).  symmetric != 0 mirrors every off-diagonal entry right after
 * the original.  Values are converted to value_type (the reference stores VALUE_TYPE, main.cpp:207). */
int csr5hip_coo_to_csr(int32_t m, int32_t n, int64_t nz, const int32_t *d_row, const int32_t *d_col,
                       const double *d_val, int symmetric, int value_type, csr5hip_csr *out);
int csr5hip_csr_release(csr5hip_csr *csr);

/* csr5hip_mtx_read + H2D + csr5hip_coo_to_csr in one call (what `./spmv foo.mtx` does first). */
int csr5hip_mtx_load(const char *path, int threads, int value_type, csr5hip_csr *out);

/* ---------------------------------------------------------------------------------------------------
 * Checkpoint of a converted matrix.  csr5hip_save writes the handle's CSR5
 * state -- row_ptr, column_index / value in tile order and the four format arrays of the reference
 * (_csr5_partition_pointer, _csr5_partition_descriptor, ..._offset_pointer, ..._offset;
 * anonymouslib_cuda.h:27-52) -- to one binary file; csr5hip_load restores it into a NEW handle that is in
 * CSR5 format at once (no conversion pass).  The CSR arrays of the loaded matrix are allocated here and
 * returned in `arrays` (the handle borrows them as after csr5hip_input_csr; release them with
 * csr5hip_csr_release AFTER csr5hip_free).  asCSR / destroy on the loaded handle give back plain CSR order.
 * ------------------------------------------------------------------------------------------------- */
int csr5hip_save(csr5hip_handle h, const char *path);
int csr5hip_load(const char *path, csr5hip_handle *h, csr5hip_csr *arrays);

/* ---------------------------------------------------------------------------------------------------
 * One matrix on the G GPUs of a node (SURVEY.md section 8, row e).  The reference is single-device
 * (CSR5_cuda/main.cu:25-26 `cudaSetDevice(0)`): this is the MI355X addition.  The matrix is cut into G contiguous
 * row blocks balanced by COST = non-zeros + row_weight * rows (split points = upper_bound(cost prefix, g*total/G) - 1,
 * the reference's tile_ptr primitive, utils_cuda.h:25-53; row_weight defaults to 2 -- what a row's y element, pointer
 * and share of the slab combine cost next to a non-zero, measured -- and CSR5HIP_MULTI_OPT_ROW_WEIGHT = 0 gives the
 * plain nnz balance); every block becomes an ordinary handle on its own device and stream; x is
 * replicated ONCE at set_x time by a single RCCL broadcast over xGMI (librccl is opened lazily; device-to-device
 * copies when it is absent or a device is listed twice); y stays sharded; no per-SpMV collective.
 * x CONTRACT of the multi handle: set_x CAPTURES x's contents.  A replica is library-owned -- the caller cannot write to
 * it -- so every shard's kernel-side (permuted) copy of x is taken once, right behind the broadcast on the shard's stream,
 * not by every spmv() (CSR5HIP_OPT_X_SNAPSHOT = 1 is the shards' default; round 6: it was 41 of each R-MAT 24 block's ~180 us).
 * The shards on devices[0] that borrow d_x follow the same contract: after writing to x call set_x again (same pointer).
 * csr5hip_multi_set_option(mh, CSR5HIP_OPT_X_SNAPSHOT, 0) restores live reads for those borrowing shards only.
 * Single host thread, all calls asynchronous per device.  devices[] may list a device several times (several
 * shards on one GPU), which is how a 1-GPU box exercises this path.
 * ------------------------------------------------------------------------------------------------- */
typedef struct csr5hip_multi_s *csr5hip_multi;

typedef struct csr5hip_shard {
    int device;              /* HIP device of the shard */
    int row_lo, row_hi;      /* global rows [row_lo, row_hi) */
    int nnz;
    void *d_y;               /* the shard's result vector on `device` (row_hi - row_lo values) */
    csr5hip_handle handle;   /* the shard's ordinary handle (csr5hip_get_info etc.) */
    int x_broadcast;         /* how the last set_x replicated x: 0 = nothing to replicate, 1 = RCCL broadcast, 2 = copies */
} csr5hip_shard;

int csr5hip_multi_create(csr5hip_multi *out, const int *devices, int G, int m, int n, int value_type);
int csr5hip_multi_free(csr5hip_multi mh);
/* inputCSR for the whole matrix: device pointers on devices[0].  Unlike the single handle the arrays are COPIED into
 * the per-device shards (and rebased); the caller's arrays are not modified by asCSR5 and may be freed afterwards. */
int csr5hip_multi_input_csr(csr5hip_multi mh, int nnz, const int32_t *d_row_ptr, const int32_t *d_col_idx, const void *d_val);
int csr5hip_multi_set_sigma(csr5hip_multi mh, int sigma);
/* csr5hip_set_option on every shard; CSR5HIP_MULTI_OPT_ROW_WEIGHT (0..64, before input_csr) is the handle's own key */
#define CSR5HIP_MULTI_OPT_ROW_WEIGHT 100
#define CSR5HIP_MULTI_DEFAULT_ROW_WEIGHT 2
/* 1 = the shards on devices[0] also read a REPLICA of x that the broadcast fills (root = devices[0] itself) instead of
 * borrowing the caller's vector: with G = 1 the one RCCL collective of this path -- communicator over the device list,
 * grouped ncclBroadcast -- then runs on a single GPU exactly as it does on eight (how the 1-GPU test box proves the
 * RCCL bindings).  Default 0.  Takes effect at the next set_x. */
#define CSR5HIP_MULTI_OPT_OWN_REPLICAS 101
int csr5hip_multi_set_option(csr5hip_multi mh, int option, int value);
int csr5hip_multi_as_csr5(csr5hip_multi mh);
/* setX: d_x on devices[0], n values, borrowed by the shards that live there; ONE broadcast to the other devices, each shard's
 * permuted copy of x (hot-table path) taken right behind it.  Call again after changing x's contents. */
int csr5hip_multi_set_x(csr5hip_multi mh, const void *d_x);
/* csr5hip_update_values for the whole matrix.  d_val_csr: the whole matrix' nnz values in CSR order on devices[0]
 * (the order input_csr's value array had); read only, not retained, must stay valid and unchanged until
 * csr5hip_multi_synchronize.  Every shard takes its contiguous slice: shards on devices[0] read it in place, a shard on
 * another device receives it by a peer copy into a staging buffer it owns (allocated on first use), then updates on its own
 * stream.  Legal only after csr5hip_multi_input_csr (CSR5HIP_UNKOWN_FORMAT before); enqueues and returns like
 * csr5hip_multi_spmv.  The shards' streams do not wait for the stream that wrote d_val_csr: synchronise it first. */
int csr5hip_multi_update_values(csr5hip_multi mh, const void *d_val_csr);
/* spmv on every shard, enqueued on the shards' streams (returns without waiting) */
int csr5hip_multi_spmv(csr5hip_multi mh, double alpha);
int csr5hip_multi_spmv_repeat(csr5hip_multi mh, double alpha, int count);
int csr5hip_multi_synchronize(csr5hip_multi mh);
/* device time between the two calls: the MAXIMUM over the shards' streams */
int csr5hip_multi_timer_start(csr5hip_multi mh);
int csr5hip_multi_timer_stop(csr5hip_multi mh, double *ms_max);
int csr5hip_multi_shard(csr5hip_multi mh, int g, csr5hip_shard *out);
/* correctness checks: the y shards collected into one HOST vector of m values; fill_y presets every y byte */
int csr5hip_multi_gather_y(csr5hip_multi mh, void *h_y);
int csr5hip_multi_fill_y(csr5hip_multi mh, int byte_value);
/* destroy() on every shard (the shards' own copies go back to CSR order) */
int csr5hip_multi_destroy(csr5hip_multi mh);

#include "csr5hip_bias.h"
#include "csr5hip_edge_bias.h"
#include "csr5hip_lowp.h"
#include "csr5hip_gat.h"
#include "csr5hip_dropout.h"
#include "csr5hip_dropout_lowp.h"
#include "csr5hip_reduce.h"

#ifdef __cplusplus
}
#endif
#endif /* CSR5HIP_H */
