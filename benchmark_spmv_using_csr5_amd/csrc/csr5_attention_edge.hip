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

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher as well.
#if !defined(CSR5_ATTENTION_ONLY_F32)
extern template AttLaunch attention_launch<AttEdgeArgs<float>>;
template AttLaunch attention_launch<AttEdgeArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttEdgeArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_edge(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttEdgeArgs<double>>(g, d, c, s);
    return attention_launch<AttEdgeArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
