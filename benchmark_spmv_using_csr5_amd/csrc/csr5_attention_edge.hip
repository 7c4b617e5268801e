// csr5_attention_edge.hip -- csr5hip_mha_edge_bias: csr5_attention.hip's packed multi-head attention with a softmax scale and an
// additive score bias taken from a CALLER-OWNED tensor B (nnz, heads) in CSR order, in ONE launch, for gfx950 (wave64):
//
//     s_e,h = fma(qk_e,h, c, B[e * ldb + h])     qk_e,h: csr5_attention.hip's chain on head h's slices, the same bits
//                                                c: the scale, converted once to the value type
//                                                e: the entry's CSR rank (row_ptr[r] + j), the order csr5hip_sddmm writes
//
// and EVERYTHING after the score is csr5_attention.hip's, per head, with these scores, as in csr5_attention_bias.hip.  These are
// the same kernel templates (csr5_attention_kern.h) instantiated with an argument struct that carries B (AttEdgeArgs); the
// plain and the biased instantiations are not touched by it.
//
// THE BIAS of an entry is read at its CSR rank, which the row kernels know without a second rank -> storage computation: a lane
// of a row of at most 16 entries keeps the rank across the heads of the workgroup and reads B[e * ldb + h] per head; the longer
// rows read it per head at every place a score is computed, the maximum sweep and every chunk refill of a row beyond 2 048
// entries included.  It is not staged in LDS, for csr5_attention_bias.hip's reason.  B is read and never written; columns
// heads .. ldb - 1 of a row of B are never read; a null B reads nothing (b = +0).  THE HANDLE'S VALUES ARE NOT READ.
//
// NON-FINITE: a -Inf bias is a hard mask of that head; otherwise as csr5_attention_bias.hip.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// groups: the head groups over grid.y, 0 for the rule (att_heads_per_group)
template <typename VT>
static hipError_t attention_edge_typed(const Geometry &g, const DeviceArrays &d, int heads, int groups, double scale, const void *B,
                                       int ldb, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,
                                       void *O, int ldo, hipStream_t s)
{
    if (g.m <= 0 || dcols <= 0 || heads <= 0)
        return hipSuccess;
    AttEdgeArgs<VT> A;
    attention_fill<VT>(A, g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo);
    A.bias.B = (const VT *)B;
    A.bias.map = nullptr;
    A.bias.ldb = ldb;
    A.bias.c = (VT)scale;
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    const dim3 grid(blocks, (unsigned)((heads + A.hper - 1) / A.hper)), block(AT_BLOCK);
    if (attention_vec<VT>(heads, Q, ldq, K, ldk, k))
        hipLaunchKernelGGL((k_attention_edge<VT, true>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((k_attention_edge<VT, false>), grid, block, 0, s, A);
    return hipGetLastError();
}

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / -DCSR5_ATTENTION_ONLY_F32), as csr5_attention.hip.
#define CSR5_EDGE_PARAMS                                                                                                                  \
    const Geometry &g, const DeviceArrays &d, int heads, int groups, double scale, const void *B, int ldb, const void *Q, int ldq,        \
        const void *K, int ldk, int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s
#define CSR5_EDGE_ARGS g, d, heads, groups, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s
#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_edge_f64(CSR5_EDGE_PARAMS) { return attention_edge_typed<double>(CSR5_EDGE_ARGS); }
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
hipError_t launch_mha_edge_f32(CSR5_EDGE_PARAMS) { return attention_edge_typed<float>(CSR5_EDGE_ARGS); }
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_edge_f32(CSR5_EDGE_PARAMS);

hipError_t launch_mha_edge(const Geometry &g, const DeviceArrays &d, int value_type, int heads, int groups, double scale, const void *B,
                           int ldb, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, void *O,
                           int ldo, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_mha_edge_f64(CSR5_EDGE_ARGS) : launch_mha_edge_f32(CSR5_EDGE_ARGS);
}
#endif
#undef CSR5_EDGE_PARAMS
#undef CSR5_EDGE_ARGS

} // namespace csr5
