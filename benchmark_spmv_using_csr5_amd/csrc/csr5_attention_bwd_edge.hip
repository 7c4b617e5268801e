// csr5_attention_bwd_edge.hip -- csr5hip_mha_edge_bias_backward: the gradients of csr5_attention_edge.hip's O for Q, K and V, and
// on request for the bias tensor B itself, in TWO launches, for gfx950 (wave64).  Per stored entry e = (i, j) and head h, every
// operation its own rounding:
//
//     s_e  = fma(qk_e, c, B[e * ldb + h]), the forward's score, the same bits (csr5_attention_edge.hip)
//     p_e, dp_e, D_i, ds_e = csr5_attention_bwd.hip's, with these scores
//     t_e  = ds_e * c                                   (one rounded multiplication)
//     dQ[i, c] = sum_e t_e K[j_e, c]      dK[j, c] = sum_e t_e Q[i_e, c]      dV[j, c] = sum_e p_e dO[i_e, c]
//     dB[e * lddb + h] = ds_e,h           (optional; the gradient of B: no reduction is needed)
//
// by csr5_attention_bwd.hip's accumulation rules, row classes, workspace and determinism contract: these are the same kernel
// templates (csr5_attention_bwd_kern.h) instantiated with an argument struct that carries B (AttBwdEdgeArgs); the plain and
// the biased instantiations are not touched by it.  THE ROW KERNEL reads B at the entry's CSR rank and writes dB exactly as the
// biased one writes dS (the extra sweep of a row beyond 2 048 entries included).  THE COLUMN KERNEL walks the transposed
// companion's pattern: the entry of rank j of companion line c sits at position q = t_row_ptr[c] + j of A^T's CSR order, and its
// rank in A's is e = map[q], map the companion's source map, which the C layer passes and nobody copies; so an entry has the
// same s, p and ds on both sides.  A lane of a short line loads e once and keeps it across the heads; the longer classes read
// the map word again per head (consecutive ranks, consecutive addresses) and then B[e * ldb + h], a scattered read.  THE
// HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher as well.
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdEdgeArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdEdgeArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdEdgeArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_edge_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdEdgeArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdEdgeArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
