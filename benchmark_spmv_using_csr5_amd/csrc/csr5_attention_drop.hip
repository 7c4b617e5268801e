// csr5_attention_drop.hip -- csr5hip_dropout_mha: csr5_attention_edge.hip's call, s = fma(qk, c, B[e * ldb + h]) with B optional, with
// DROPOUT ON THE ATTENTION WEIGHTS, after the softmax and before the product with V, in the same ONE launch, for gfx950 (wave64); and
// csr5hip_dropout_mask, the mask itself.  Per stored entry e (its CSR rank in the parent's pattern) and absolute head g = head0 + h:
//
//     dropped = philox4x32_10((e, g >> 2, offset low, offset high), (seed low, seed high))[g & 3] < thr
//     thr     = min(llrint(p 2^32), 2^32 - 1)           cd = (VT)(1 / (1 - p)), both formed once on the host
//     M, w_e, Z = the undropped call's: the softmax is over ALL stored entries, dropped ones included
//     O[i, h, :] = (sum over the row's entries of fma(keep ? w_e : +0, V[j, h, :], acc)) * (rinv * cd)
//
// rinv * cd is one rounded multiplication per row and head; the summation orders, the row classes and the head groups are
// csr5_attention.hip's.  A dropped weight still goes through the FMA, as a -Inf-masked entry's does.  With p = 0 (thr = 0, cd = 1)
// every bit is csr5hip_mha_edge_bias's.  These are the same kernel templates (csr5_attention_kern.h) instantiated with an argument
// struct derived from the edge one (AttDropArgs: ARGS::DROP); no other instantiation is touched by it.  The mask is a pure function of
// (seed, offset, e, g): the backward recomputes it (csr5_attention_bwd_drop.hip), nothing of length nnz is written.
// THE HANDLE'S VALUES ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher and the mask kernel as well.
#if !defined(CSR5_ATTENTION_ONLY_F32)
extern template AttLaunch attention_launch<AttDropArgs<float>>;
template AttLaunch attention_launch<AttDropArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttDropArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_drop(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttDropArgs<double>>(g, d, c, s);
    return attention_launch<AttDropArgs<float>>(g, d, c, s);
}

// one byte per (entry, head): 1 kept, 0 dropped.  A thread owns one entry and walks its heads; total = nnz entries
__global__ void __launch_bounds__(AT_BLOCK) k_dropout_mask(const AttDropKey key, const int nnz, const int heads, unsigned char *mask,
                                                      const int ldm)
{
    const long long e = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;
    if (e >= nnz)
        return;
    for (int h = 0; h < heads; h++)
        mask[(size_t)e * (size_t)ldm + (size_t)h] = att_drop_keep(key, (size_t)e, h) ? 1 : 0;
}

hipError_t launch_dropout_mask(int nnz, const AttCall &c, unsigned char *mask, int ldm, hipStream_t s)
{
    if (nnz <= 0 || c.heads <= 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)nnz + AT_BLOCK - 1) / AT_BLOCK);
    hipLaunchKernelGGL(k_dropout_mask, dim3(blocks), dim3(AT_BLOCK), 0, s, att_drop_key(c), nnz, c.heads, mask, ldm);
    return hipGetLastError();
}
#endif

} // namespace csr5
