// csr5_companion.hip -- the transposed companion of a converted matrix: a CSR of A^T built on the device from the tile-ordered
// arrays of a CSR5 handle (csr5hip_build_transpose).
//
// Canonical A^T: row j holds A's entries of column j in ascending order of their position in A's CSR arrays -- what a STABLE
// sort of the CSR column array gives.  Steps:
//   k_companion_keys    key[c] = column of A's c-th element in CSR order, read from the tile-ordered column_index through the
//                       tile transpose map (as k_refresh_keys of csr5_refresh.hip; the tail tile is in CSR order already)
//   radix_sort_pairs    stable, over ceil(log2 n) key bits, payload = CSR position: the sorted payload IS the source map
//                       (position in A^T's CSR -> position in A's CSR) that csr5hip_update_values needs
//   k_companion_rowptr  row pointer of A^T: a lower bound of every j in 0 .. n in the sorted keys (empty columns included)
//   k_companion_fill    per element of A^T: its column = the row of A that owns the source position (search in row_ptr), its
//                       value = A's value at the source position's place in the tile-ordered value array
// k_companion_gather is the per-update half: stage[q] = new_values[map[q]].
// Value-type independent: values are moved as 4- or 8-byte words.
#include "csr5_internal.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

namespace csr5 {

// one thread per STORAGE position of the tile-ordered column_index
__global__ void __launch_bounds__(256) k_companion_keys(Geometry g, const uint32_t *__restrict__ tile_ptr,
                                                        const int32_t *__restrict__ col, uint32_t *__restrict__ key)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)g.nnz)
        return;
    const int T = g.tile_elems;
    const int t = (int)(q / (size_t)T), idx = (int)(q - (size_t)t * T);
    const bool tr = t < g.p - 1 && tile_ptr[t] != tile_ptr[t + 1];
    const int c = tr ? (idx & (OMEGA - 1)) * g.sigma + (idx >> 6) : idx;
    key[(size_t)t * T + c] = (uint32_t)col[q];
}

// row_ptr_t[j] = number of sorted keys < j, j = 0 .. n
__global__ void __launch_bounds__(256) k_companion_rowptr(int n, int nnz, const uint32_t *__restrict__ key_sorted,
                                                          int32_t *__restrict__ row_ptr_t)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j > n)
        return;
    int lo = 0, hi = nnz; // first position in [0, nnz] whose key is >= j
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (key_sorted[mid] < (uint32_t)j)
            lo = mid + 1;
        else
            hi = mid;
    }
    row_ptr_t[j] = lo;
}

// storage position of A's c-th element in CSR order (the inverse of k_companion_keys' map)
__device__ __forceinline__ size_t companion_storage_of(const Geometry &g, const uint32_t *__restrict__ tile_ptr, uint32_t c)
{
    const int T = g.tile_elems;
    const int t = (int)(c / (uint32_t)T), idx = (int)(c - (uint32_t)t * (uint32_t)T);
    const bool tr = t < g.p - 1 && tile_ptr[t] != tile_ptr[t + 1];
    if (!tr)
        return (size_t)c;
    const int l = idx / g.sigma, i = idx - l * g.sigma; // CSR rank l * sigma + i -> (step i, lane l)
    return (size_t)t * T + (size_t)i * OMEGA + l;
}

// one thread per element of A^T in CSR order
template <typename W>
__global__ void __launch_bounds__(256) k_companion_fill(Geometry g, const uint32_t *__restrict__ tile_ptr,
                                                        const int32_t *__restrict__ row_ptr, const uint32_t *__restrict__ map,
                                                        const W *__restrict__ val, int32_t *__restrict__ col_t,
                                                        W *__restrict__ val_t)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (size_t)g.nnz)
        return;
    const uint32_t c = map[q];
    int lo = 0, hi = g.m; // the row r with row_ptr[r] <= c < row_ptr[r + 1]: first index in [0, m] whose pointer is > c, minus 1
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)row_ptr[mid + 1] <= c)
            lo = mid + 1;
        else
            hi = mid;
    }
    col_t[q] = lo < g.m ? lo : g.m - 1; // (a valid row_ptr ends at nnz > c: the clamp never acts on one)
    val_t[q] = val[companion_storage_of(g, tile_ptr, c)];
}

template <typename W>
__global__ void __launch_bounds__(256) k_companion_gather(int nnz, const uint32_t *__restrict__ map, const W *__restrict__ in,
                                                          W *__restrict__ out)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < (size_t)nnz)
        out[q] = in[map[q]];
}

int companion_key_bits(int n)
{
    int bits = 1;
    while (bits < 31 && (1LL << bits) < (long long)n)
        bits++;
    return bits;
}

// temporaries of companion_build: the keys in and out (4 bytes per non-zero each), then the sort's own storage
static size_t companion_key_bytes(int nnz) { return ((size_t)nnz * 4 + 255) & ~(size_t)255; }
hipError_t companion_tmp_bytes(int n, int nnz, size_t *bytes)
{
    size_t sort_bytes = 0;
    uint32_t *null_k = nullptr, *null_v = nullptr;
    const hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, null_k, null_k, rocprim::counting_iterator<uint32_t>(0u),
                                                   null_v, (size_t)nnz, 0u, (unsigned)companion_key_bits(n), nullptr);
    *bytes = 2 * companion_key_bytes(nnz) + sort_bytes;
    return e;
}

// g / d: the PARENT in CSR5 form.  row_ptr_t [n + 1], col_t [nnz], val_t [nnz values], map [nnz] <- the CSR of A^T and its source map
hipError_t companion_build(const Geometry &g, const DeviceArrays &d, int value_size, void *tmp, size_t tmp_bytes,
                           int32_t *row_ptr_t, int32_t *col_t, void *val_t, uint32_t *map, hipStream_t s)
{
    if (g.nnz <= 0)
        return hipSuccess;
    const size_t kb = companion_key_bytes(g.nnz);
    if (tmp_bytes < 2 * kb || (value_size != 4 && value_size != 8))
        return hipErrorInvalidValue;
    uint32_t *key_in = (uint32_t *)tmp, *key_out = (uint32_t *)((char *)tmp + kb);
    size_t sort_bytes = tmp_bytes - 2 * kb;
    const dim3 per_nnz((unsigned)(((size_t)g.nnz + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_companion_keys, per_nnz, block, 0, s, g, d.tile_ptr, d.col, key_in);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    // stable: inside a column the elements keep their CSR order
    e = rocprim::radix_sort_pairs((void *)((char *)tmp + 2 * kb), sort_bytes, key_in, key_out, rocprim::counting_iterator<uint32_t>(0u),
                                  map, (size_t)g.nnz, 0u, (unsigned)companion_key_bits(g.n), s);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_companion_rowptr, dim3((unsigned)(((size_t)g.n + 1 + 255) / 256)), block, 0, s, g.n, g.nnz, key_out, row_ptr_t);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (value_size == 8)
        hipLaunchKernelGGL((k_companion_fill<uint64_t>), per_nnz, block, 0, s, g, d.tile_ptr, d.row_ptr, map, (const uint64_t *)d.val,
                           col_t, (uint64_t *)val_t);
    else
        hipLaunchKernelGGL((k_companion_fill<uint32_t>), per_nnz, block, 0, s, g, d.tile_ptr, d.row_ptr, map, (const uint32_t *)d.val,
                           col_t, (uint32_t *)val_t);
    return hipGetLastError();
}

// out[q] = in[map[q]], q < nnz: new values (A's CSR order) into A^T's CSR order
hipError_t companion_gather(int nnz, int value_size, const uint32_t *map, const void *in, void *out, hipStream_t s)
{
    if (nnz <= 0)
        return hipSuccess;
    const dim3 grid((unsigned)(((size_t)nnz + 255) / 256)), block(256);
    if (value_size == 8)
        hipLaunchKernelGGL((k_companion_gather<uint64_t>), grid, block, 0, s, nnz, map, (const uint64_t *)in, (uint64_t *)out);
    else
        hipLaunchKernelGGL((k_companion_gather<uint32_t>), grid, block, 0, s, nnz, map, (const uint32_t *)in, (uint32_t *)out);
    return hipGetLastError();
}

} // namespace csr5
