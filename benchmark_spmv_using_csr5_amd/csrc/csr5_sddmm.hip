// csr5_sddmm.hip -- sampled dense-dense product on the CSR5 pattern for gfx950 (wave64):
//     out[e] = sum_{c < k} U[row(e), c] * V[col(e), c]      for every stored element e of A, out in CSR order.
//
// U is m x k and V is n x k, both row-major with leading dimensions ldu / ldv.  The matrix values play no part.  One wavefront
// walks one tile of the plain (parent) tile structure, as k_spmv / k_spmm do; nothing but the structure is read:
//
//   row of an element   tiles 0 .. p-2: element (lane l, step i) lies in the row that the cnt-th row start of the tile opens,
//                       cnt = y_offset(l) + number of the lane's bit flags at steps 0 .. i (lane 0's forced first flag is not a
//                       row start of the tile and is not counted).  cnt = 0: row_start = tile_ptr[t] & ROW_MASK; otherwise
//                       row_start + 1 + (cnt - 1), or, for a tile with empty rows (bit 31 of tile_ptr[t]),
//                       row_start + 1 + offset[offset_ptr[t] + cnt - 1].  This is where k_spmv stores the segment that the
//                       element belongs to (csr5_format.hip numbers the flags the same way).  A tile whose two masked tile_ptr words
//                       are equal lies inside row_start.  No search in row_ptr, no row index per element.
//                       tail tile p-1: one thread per row tail_start .. m-1 walks row_ptr[r] .. row_ptr[r+1] (clamped to the
//                       tail), rows of more than 32 elements are walked by the whole wavefront.
//   column              the tile-ordered column_index: element (l, i) of tile t at t T + i 64 + l
//   CSR rank            moved tiles (raw tile_ptr words differ): t T + l sigma + i, so a lane's sigma outputs are contiguous
//                       and every group of SDDMM_GROUP of them is stored as one run; fast-track tiles (raw words equal) and the
//                       tail are stored in CSR order: rank = storage position.
//
// Blocking: a lane takes its elements in groups of SDDMM_GROUP (their dot products are independent chains), and the k columns
// in blocks of 32 bytes per row (4 fp64 / 8 fp32): two 16-byte loads of the U row and of the gathered V row per block when
// U, V, ldu and ldv allow, element loads otherwise and for the remainder block.  Neighbouring elements of a lane mostly share
// their U row: those loads hit in the L1.  No k-wide register array: 2 x SDDMM_GROUP x 32 bytes of operands are live.
//
// DETERMINISM CONTRACT.  out[e] = fma(u[k-1], v[k-1], ... fma(u[1], v[1], fma(u[0], v[0], +0)) ...): ONE chain of k fused
// multiply-adds in ascending column order onto +0, every product unrounded inside its FMA.  out[e] depends only on the k
// values of U's row, the k values of V's row, k and the value type -- not on sigma, any handle option, the element's position
// or tile kind, ldu / ldv, pointer alignment (vector and element loads feed the same chain) or the run.  k = 0 gives +0.
// A dot product is computed from its own two rows only: masked columns of a remainder block are skipped by a select, never
// multiplied by zero, so Inf / NaN stay where they are; nothing is flushed.  No atomics, no LDS, nothing allocated.
#include "csr5_internal.h"
#include "csr5_wave.h"

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

namespace csr5 {

constexpr int SDDMM_GROUP = 4;      // elements of a lane whose chains run side by side
constexpr int SDDMM_ROW_BYTES = 32; // column block: bytes of a U row and of a V row per step
constexpr int SDDMM_LONG_ROW = 32;  // tail rows beyond this many elements are walked by the whole wavefront

template <typename VT>
__device__ __forceinline__ void sddmm_load16(const VT *__restrict__ p, VT *o)
{
    const uint4 w = *reinterpret_cast<const uint4 *>(p);
    if constexpr (sizeof(VT) == 8) {
        o[0] = __builtin_bit_cast(double, (unsigned long long)w.y << 32 | w.x);
        o[1] = __builtin_bit_cast(double, (unsigned long long)w.w << 32 | w.z);
    } else {
        o[0] = __builtin_bit_cast(float, w.x);
        o[1] = __builtin_bit_cast(float, w.y);
        o[2] = __builtin_bit_cast(float, w.z);
        o[3] = __builtin_bit_cast(float, w.w);
    }
}

// acc[e] = the chain of the contract over rows u[e], v[e], for G independent elements.  VEC: whole blocks by 16-byte loads.
template <typename VT, bool VEC, int G>
__device__ __forceinline__ void sddmm_dots(const VT *const (&u)[G], const VT *const (&v)[G], const int k, VT (&acc)[G])
{
    constexpr int KB = SDDMM_ROW_BYTES / (int)sizeof(VT);
    constexpr int PER = 16 / (int)sizeof(VT);
#pragma unroll
    for (int e = 0; e < G; e++)
        acc[e] = (VT)0;
    int c = 0;
    if constexpr (VEC) {
        for (; c + KB <= k; c += KB) {
            VT ub[G][KB], vb[G][KB];
#pragma unroll
            for (int e = 0; e < G; e++) {
#pragma unroll
                for (int q = 0; q < KB / PER; q++) {
                    sddmm_load16<VT>(u[e] + c + q * PER, &ub[e][q * PER]);
                    sddmm_load16<VT>(v[e] + c + q * PER, &vb[e][q * PER]);
                }
            }
#pragma unroll
            for (int j = 0; j < KB; j++) {
#pragma unroll
                for (int e = 0; e < G; e++)
                    acc[e] = fma_vt(ub[e][j], vb[e][j], acc[e]);
            }
        }
    }
    for (; c < k; c += KB) {
        const int kc = k - c < KB ? k - c : KB;
        VT ub[G][KB], vb[G][KB];
#pragma unroll
        for (int e = 0; e < G; e++) {
#pragma unroll
            for (int j = 0; j < KB; j++) {
                ub[e][j] = j < kc ? u[e][c + j] : (VT)0;
                vb[e][j] = j < kc ? v[e][c + j] : (VT)0;
            }
        }
#pragma unroll
        for (int j = 0; j < KB; j++) {
#pragma unroll
            for (int e = 0; e < G; e++) {
                const VT next = fma_vt(ub[e][j], vb[e][j], acc[e]);
                acc[e] = j < kc ? next : acc[e]; // a masked column is skipped, not multiplied by zero
            }
        }
    }
}

// ---- CSR tail: rows tail_start .. m-1, one thread per row, long rows by the whole wavefront -------------------------------
template <typename VT, bool VEC>
__device__ __forceinline__ void sddmm_tail(const Geometry &g, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                           const VT *__restrict__ U, const int ldu, const VT *__restrict__ V, const int ldv,
                                           const int k, VT *__restrict__ out, const int tail_block)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    const int first_tail = (g.p - 1) * g.tile_elems;
    const int r = g.tail_start + tail_block * BLOCK + (int)threadIdx.x;
    const bool valid = r < g.m;
    int a = 0, b = 0;
    if (valid) {
        a = row_ptr[r];
        b = row_ptr[r + 1];
        a = a < first_tail ? first_tail : a; // (the first tail row may have begun before the tail)
        b = b < a ? a : b;
    }
    const bool longrow = b - a > SDDMM_LONG_ROW;
    if (!longrow) {
        const VT *const ur[1] = {U + (size_t)(valid ? r : 0) * ldu};
        for (int e = a; e < b; e++) {
            const VT *const vr[1] = {V + (size_t)(uint32_t)col[e] * ldv};
            VT acc[1];
            sddmm_dots<VT, VEC, 1>(ur, vr, k, acc);
            out[e] = acc[0];
        }
    }
    unsigned long long todo = __ballot(longrow);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int aa = __shfl(a, src, OMEGA);
        const int bb = __shfl(b, src, OMEGA);
        const int rr = __shfl(r, src, OMEGA);
        const VT *const ur[1] = {U + (size_t)rr * ldu};
        for (int e = aa + lane; e < bb; e += OMEGA) {
            const VT *const vr[1] = {V + (size_t)(uint32_t)col[e] * ldv};
            VT acc[1];
            sddmm_dots<VT, VEC, 1>(ur, vr, k, acc);
            out[e] = acc[0];
        }
    }
}

// ---- tiles 0 .. p-2: one tile per wavefront, sigma at run time (the walk is a shift and a population count per element) ---
template <typename VT, bool VEC>
__global__ void __launch_bounds__(BLOCK)
k_sddmm(Geometry g, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const uint32_t *__restrict__ tile_ptr,
        const uint32_t *__restrict__ tile_desc, const int32_t *__restrict__ offset_ptr, const int32_t *__restrict__ offset,
        const VT *__restrict__ U, int ldu, const VT *__restrict__ V, int ldv, int k, VT *__restrict__ out, int tile_blocks)
{
    const int blk = blockIdx.x;
    if (blk >= tile_blocks) {
        sddmm_tail<VT, VEC>(g, row_ptr, col, U, ldu, V, ldv, k, out, blk - tile_blocks);
        return;
    }
    const int lane = threadIdx.x & (OMEGA - 1);
    const int t = __builtin_amdgcn_readfirstlane(blk * WAVES_PER_BLOCK + (int)(threadIdx.x >> 6));
    if (t >= g.p - 1)
        return;
    const int sigma = g.sigma;
    const int bit_y = g.bit_y;
    const int bit_all = bit_y + BIT_SS;
    const uint32_t tp0 = tile_ptr[t];
    const uint32_t tp1 = tile_ptr[t + 1];
    const bool moved = tp0 != tp1;                            // transposed storage (csr5_format.hip k_transpose)
    const bool one_row = (tp0 & ROW_MASK) == (tp1 & ROW_MASK); // the whole tile inside row_start: its descriptor holds raw flags only
    const bool empty_rows = (bool)(tp0 >> 31) && !one_row;
    const int row_start = (int)(tp0 & ROW_MASK);
    const uint32_t *d = tile_desc + (size_t)t * OMEGA * g.num_packet;
    const uint32_t w0 = d[lane];
    const uint32_t w1 = g.num_packet > 1 ? d[OMEGA + lane] : 0u;
    uint32_t flags = w0 << bit_all; // step i -> bit 31-i
    if (g.num_packet > 1)
        flags |= w1 >> (32 - bit_all);
    if (lane == 0)
        flags &= 0x7FFFFFFFu; // (a row that starts exactly on the tile boundary IS row_start)
    if (one_row)
        flags = 0;
    const int y_off = one_row ? 0 : (int)(w0 >> (32 - bit_y));
    const int32_t *off_local = empty_rows ? offset + offset_ptr[t] : nullptr;
    const size_t base = (size_t)t * g.tile_elems;
    const int32_t *ct = col + base + lane;
    VT *ot = out + base + (moved ? (size_t)lane * sigma : (size_t)lane);
    const int ostep = moved ? 1 : OMEGA;

    for (int i0 = 0; i0 < sigma; i0 += SDDMM_GROUP) {
        const VT *ur[SDDMM_GROUP];
        const VT *vr[SDDMM_GROUP];
#pragma unroll
        for (int e = 0; e < SDDMM_GROUP; e++) {
            const int i = i0 + e < sigma ? i0 + e : sigma - 1; // (a step beyond sigma repeats the last one and is not stored)
            const int32_t cw = ct[(size_t)i * OMEGA];
            const int cnt = y_off + __builtin_popcount(flags >> (31 - i));
            int rel = 0;
            if (cnt > 0)
                rel = 1 + (empty_rows ? off_local[cnt - 1] : cnt - 1);
            ur[e] = U + (size_t)(row_start + rel) * ldu;
            vr[e] = V + (size_t)(uint32_t)cw * ldv;
        }
        VT acc[SDDMM_GROUP];
        sddmm_dots<VT, VEC, SDDMM_GROUP>(ur, vr, k, acc);
#pragma unroll
        for (int e = 0; e < SDDMM_GROUP; e++)
            if (i0 + e < sigma)
                ot[(size_t)(i0 + e) * ostep] = acc[e];
    }
}

template <typename VT>
static hipError_t sddmm_typed(const Geometry &g, const DeviceArrays &d, const void *U, int ldu, const void *V, int ldv, int k,
                              void *out, hipStream_t s)
{
    if (g.p <= 0 || g.nnz <= 0)
        return hipSuccess;
    const int tile_blocks = g.p > 1 ? (g.p - 1 + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK : 0;
    const int tail_rows_n = g.m - g.tail_start;
    const int tail_blocks = tail_rows_n > 0 ? (tail_rows_n + BLOCK - 1) / BLOCK : 0;
    if (tile_blocks + tail_blocks == 0)
        return hipSuccess;
    // 16-byte loads: at least one whole block, and every row of U and of V starts on a 16-byte boundary
    const bool vec = k >= SDDMM_ROW_BYTES / (int)sizeof(VT) && reinterpret_cast<uintptr_t>(U) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(V) % 16 == 0 && ((size_t)ldu * sizeof(VT)) % 16 == 0 &&
                     ((size_t)ldv * sizeof(VT)) % 16 == 0;
    const dim3 grid((unsigned)(tile_blocks + tail_blocks)), block(BLOCK);
    if (vec)
        hipLaunchKernelGGL((k_sddmm<VT, true>), grid, block, 0, s, g, d.row_ptr, d.col, d.tile_ptr, d.tile_desc, d.offset_ptr, d.offset,
                           (const VT *)U, ldu, (const VT *)V, ldv, k, (VT *)out, tile_blocks);
    else
        hipLaunchKernelGGL((k_sddmm<VT, false>), grid, block, 0, s, g, d.row_ptr, d.col, d.tile_ptr, d.tile_desc, d.offset_ptr, d.offset,
                           (const VT *)U, ldu, (const VT *)V, ldv, k, (VT *)out, tile_blocks);
    return hipGetLastError();
}

// The product build compiles this file once per value type (-DCSR5_SDDMM_ONLY_F64 / -DCSR5_SDDMM_ONLY_F32), as csr5_spmm.hip.
#if !defined(CSR5_SDDMM_ONLY_F32)
hipError_t launch_sddmm_f64(const Geometry &g, const DeviceArrays &d, const void *U, int ldu, const void *V, int ldv, int k, void *out,
                            hipStream_t s)
{
    return sddmm_typed<double>(g, d, U, ldu, V, ldv, k, out, s);
}
#endif
#if !defined(CSR5_SDDMM_ONLY_F64)
hipError_t launch_sddmm_f32(const Geometry &g, const DeviceArrays &d, const void *U, int ldu, const void *V, int ldv, int k, void *out,
                            hipStream_t s)
{
    return sddmm_typed<float>(g, d, U, ldu, V, ldv, k, out, s);
}
#endif

#if !defined(CSR5_SDDMM_ONLY_F32)
hipError_t launch_sddmm_f32(const Geometry &g, const DeviceArrays &d, const void *U, int ldu, const void *V, int ldv, int k, void *out,
                            hipStream_t s);

hipError_t launch_sddmm(const Geometry &g, const DeviceArrays &d, int value_type, const void *U, int ldu, const void *V, int ldv, int k,
                        void *out, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_sddmm_f64(g, d, U, ldu, V, ldv, k, out, s)
                                     : launch_sddmm_f32(g, d, U, ldu, V, ldv, k, out, s);
}
#endif

} // namespace csr5
