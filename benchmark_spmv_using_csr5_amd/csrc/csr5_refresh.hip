// csr5_refresh.hip -- csr5hip_update_values: new numerical values for a converted matrix, every pattern-derived array kept.
//
// Three arrays of a CSR5 handle depend on the values:
//   the parent's `val`            tiles 0 .. p-2 whose raw tile_ptr words differ: sigma x 64 transposed (csr5_format.hip
//                                 k_transpose), fast-track tiles and the tail tile p-1 in CSR order
//   the slab child's `val`        the same layout at the child's sigma (plain child), or lane-major 16-byte pieces on EVERY
//                                 tile 0 .. p'-2 (hot child, k_transpose_values); its CSR order is the stable partition of the
//                                 parent's non-zeros by slab_of(column)
//   the child's fp32 copy         launch_fp32_exact + launch_narrow (csr5_hot.hip) on the child's new values, unchanged
// k_refresh_values writes the first two OUT OF PLACE from the caller's CSR-ordered array: a workgroup reads its tiles in the
// destination's CSR order (coalesced; through the source map for a child), stages them in LDS at the transposed position
// (the pitch of k_transpose) and stores them in storage order, coalesced.  2 x sizeof(vT) bytes per non-zero, + 4 for the map.
//
// The source map of a child -- src[q] = parent CSR rank of the child's q-th element in CSR order -- depends on the column
// indices only.  It is built once per conversion by the first update: the slab of every parent element in CSR order
// (k_refresh_keys reads the tile-ordered column_index through the transpose map), then a STABLE radix sort of
// (slab, rank) pairs over the log2(S) slab bits: exactly the order k_slab_scatter produces.
#include "csr5_internal.h"
#include "csr5_slabmap.h"

#if !defined(CSR5_REFRESH_ONLY_F32)
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#endif

namespace csr5 {

// the LDS pitch of k_transpose (csr5_format.hip transpose_pitch): 64 consecutive CSR ranks spread over all banks
__host__ __device__ inline int refresh_pitch(int sigma) { return OMEGA + (OMEGA / sigma > 0 ? OMEGA / sigma : 1); }

// n / sigma without a hardware division (the kernel is element-wise: three run-time divisions per element and phase bound it at
// 4-byte values): sigma's reciprocal in 20 fractional bits, rounded up.  With m = (2^20 + e) / sigma, 0 < e <= sigma, the quotient
// (n * m) >> 20 is exact while n * e < 2^20; here n < 2048 (an element's position in its tile, a chunk's in its workgroup) and
// sigma <= 32.
__device__ __forceinline__ unsigned refresh_div(unsigned n, unsigned recip) { return (n * recip) >> 20; }

// PIECES = false: element (lane l, step i) of a moved tile at i * 64 + l, moved = the tile_ptr words differ (k_transpose)
// PIECES = true : piece q of lane l (its elements q PER .. q PER + PER - 1, PER = 16 / sizeof(VT)) at (q * 64 + l) * PER,
//                 every tile 0 .. p-2 moved (k_transpose_values; sigma is a multiple of PER)
// MAPPED: element j of the destination's CSR order is in[src[j]], else in[j]
template <typename VT, bool PIECES, bool MAPPED>
__global__ void __launch_bounds__(FMT_BLOCK)
k_refresh_values(Geometry g, const uint32_t *__restrict__ tile_ptr, const uint32_t *__restrict__ src,
                 const VT *__restrict__ in, VT *__restrict__ out, int tiles_per_block)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    VT *sv = reinterpret_cast<VT *>(smem);
    __shared__ int moved[16]; // (tiles_per_block <= 16)
    const int t0 = blockIdx.x * tiles_per_block;
    const int T = g.tile_elems, sigma = g.sigma;
    const int pitch = refresh_pitch(sigma);
    const int per_tile = sigma * pitch;
    const unsigned recip = (1u << 20) / (unsigned)sigma + 1u;
    if ((int)threadIdx.x < tiles_per_block) {
        const int t = t0 + (int)threadIdx.x;
        moved[threadIdx.x] = t < g.p - 1 && (PIECES || tile_ptr[t] != tile_ptr[t + 1]);
    }
    __syncthreads();
    const size_t base = (size_t)t0 * T;
    const size_t nnz = (size_t)g.nnz;
    const int total = tiles_per_block * T;
    for (int e = threadIdx.x; e < total; e += FMT_BLOCK) {
        if (base + e >= nnz)
            break; // (only the tail tile is partial, and a thread's positions ascend)
        const VT v = MAPPED ? in[src[base + e]] : in[base + e];
        const int tt = (int)refresh_div((unsigned)e >> 6, recip), idx = e - tt * T; // (T = 64 sigma)
        const int l = (int)refresh_div((unsigned)idx, recip), i = idx - l * sigma;  // CSR rank l * sigma + i -> (step i, lane l)
        if (moved[tt])
            sv[tt * per_tile + i * pitch + l] = v;
        else
            out[base + e] = v; // fast-track tile / tail: CSR order
    }
    __syncthreads();
    constexpr int PER = 16 / (int)sizeof(VT);
    for (int e = threadIdx.x; e < total; e += FMT_BLOCK) {
        const int tt = (int)refresh_div((unsigned)e >> 6, recip), idx = e - tt * T;
        if (!moved[tt]) // (a moved tile is a whole tile below nnz)
            continue;
        int i, l;
        if (PIECES) {
            const int piece = idx / PER;
            l = piece & (OMEGA - 1);
            i = (piece >> 6) * PER + idx % PER;
        } else {
            l = idx & (OMEGA - 1);
            i = idx >> 6;
        }
        out[base + e] = sv[tt * per_tile + i * pitch + l];
    }
}

template <typename VT>
static hipError_t launch_refresh_typed(const Geometry &g, const uint32_t *tile_ptr, bool pieces, const uint32_t *src, const void *in,
                                void *out, hipStream_t s)
{
    if (g.p <= 0 || g.nnz <= 0)
        return hipSuccess;
    if (g.sigma < 1 || g.sigma > CSR5HIP_MAX_SIGMA || (pieces && g.sigma % (16 / (int)sizeof(VT)) != 0))
        return hipErrorInvalidValue; // (refresh_div is exact up to sigma = 32)
    // ~12 KB of values per workgroup, as k_transpose stages (one tile at sigma = 16 fp64 + its columns there)
    int tpb = (int)(12288 / ((size_t)g.tile_elems * sizeof(VT)));
    tpb = tpb < 1 ? 1 : (tpb > 16 ? 16 : tpb);
    const size_t lds = (size_t)tpb * g.sigma * refresh_pitch(g.sigma) * sizeof(VT);
    const dim3 grid((unsigned)((g.p + tpb - 1) / tpb)), block(FMT_BLOCK);
#define CSR5_REFRESH(P, M)                                                                                            \
    hipLaunchKernelGGL((k_refresh_values<VT, P, M>), grid, block, lds, s, g, tile_ptr, src, (const VT *)in, (VT *)out, tpb)
    if (pieces) {
        if (src)
            CSR5_REFRESH(true, true);
        else
            CSR5_REFRESH(true, false);
    } else {
        if (src)
            CSR5_REFRESH(false, true);
        else
            CSR5_REFRESH(false, false);
    }
#undef CSR5_REFRESH
    return hipGetLastError();
}

// The product build compiles this file once per value type (-DCSR5_REFRESH_ONLY_F64 / -DCSR5_REFRESH_ONLY_F32), like csr5_spmv.hip.
#if !defined(CSR5_REFRESH_ONLY_F32)
hipError_t launch_refresh_f64(const Geometry &g, const uint32_t *tile_ptr, bool pieces, const uint32_t *src, const void *in, void *out,
                              hipStream_t s)
{
    return launch_refresh_typed<double>(g, tile_ptr, pieces, src, in, out, s);
}
#endif
#if !defined(CSR5_REFRESH_ONLY_F64)
hipError_t launch_refresh_f32(const Geometry &g, const uint32_t *tile_ptr, bool pieces, const uint32_t *src, const void *in, void *out,
                              hipStream_t s)
{
    return launch_refresh_typed<float>(g, tile_ptr, pieces, src, in, out, s);
}
#endif

#if !defined(CSR5_REFRESH_ONLY_F32)
hipError_t launch_refresh_f32(const Geometry &g, const uint32_t *tile_ptr, bool pieces, const uint32_t *src, const void *in, void *out,
                              hipStream_t s);

hipError_t launch_refresh_values(const Geometry &g, const uint32_t *tile_ptr, int value_type, bool pieces, const uint32_t *src,
                                 const void *in, void *out, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_refresh_f64(g, tile_ptr, pieces, src, in, out, s)
                                     : launch_refresh_f32(g, tile_ptr, pieces, src, in, out, s);
}

// ---- the source map of a slab child (value-type independent) -------------------------------------------------------------
// key[j] = slab of the parent's j-th element in CSR order; one thread per STORAGE position of the tile-ordered column_index
__global__ void __launch_bounds__(256) k_refresh_keys(Geometry g, const uint32_t *__restrict__ tile_ptr,
                                                      const int32_t *__restrict__ col, int bits, int shift,
                                                      uint8_t *__restrict__ key)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)g.nnz)
        return;
    const int T = g.tile_elems;
    const int t = (int)(q / (size_t)T), idx = (int)(q - (size_t)t * T);
    const bool tr = t < g.p - 1 && tile_ptr[t] != tile_ptr[t + 1];
    const int c = tr ? (idx & (OMEGA - 1)) * g.sigma + (idx >> 6) : idx;
    key[(size_t)t * T + c] = (uint8_t)slab_of((uint32_t)col[q], shift, bits);
}

// temporaries of refresh_build_map: the keys in and out (one byte per non-zero each), then the sort's own storage
static size_t refresh_key_bytes(int nnz) { return ((size_t)nnz + 255) & ~(size_t)255; }
hipError_t refresh_map_tmp_bytes(int nnz, int bits, size_t *bytes)
{
    size_t sort_bytes = 0;
    uint8_t *null_k = nullptr;
    uint32_t *null_v = nullptr;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, null_k, null_k, rocprim::counting_iterator<uint32_t>(0u),
                                                   null_v, (size_t)nnz, 0u, (unsigned)bits, nullptr);
    *bytes = 2 * refresh_key_bytes(nnz) + sort_bytes;
    return e;
}

// g / d: the PARENT in CSR5 form (column_index in tile order); src [nnz] <- parent CSR rank of every child element
hipError_t refresh_build_map(const Geometry &g, const DeviceArrays &d, int bits, int shift, void *tmp, size_t tmp_bytes,
                             uint32_t *src, hipStream_t s)
{
    if (g.nnz <= 0)
        return hipSuccess;
    const size_t kb = refresh_key_bytes(g.nnz);
    if (tmp_bytes < 2 * kb)
        return hipErrorInvalidValue;
    uint8_t *key_in = (uint8_t *)tmp, *key_out = key_in + kb;
    size_t sort_bytes = tmp_bytes - 2 * kb;
    hipLaunchKernelGGL(k_refresh_keys, dim3((unsigned)(((size_t)g.nnz + 255) / 256)), dim3(256), 0, s, g, d.tile_ptr, d.col, bits,
                       shift, key_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    // stable: inside a slab the elements keep their CSR order, as in k_slab_scatter
    return rocprim::radix_sort_pairs((void *)(key_out + kb), sort_bytes, key_in, key_out, rocprim::counting_iterator<uint32_t>(0u), src,
                                     (size_t)g.nnz, 0u, (unsigned)bits, s);
}
#endif

} // namespace csr5
