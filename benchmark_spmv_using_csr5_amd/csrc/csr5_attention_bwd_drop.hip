// csr5_attention_bwd_drop.hip -- csr5hip_dropout_mha_backward: the gradients of csr5_attention_drop.hip's O for Q, K, V and, on request,
// the bias tensor B, in TWO launches, for gfx950 (wave64).  Both kernels recompute the forward's mask from the entry's rank in the
// PARENT's CSR order -- the position walked in the row kernel, the companion's source map word in the column kernel -- so an entry
// has the same g on both sides.  Per stored entry e = (i, j) and head h, every operation its own rounding:
//
//     g_e  = keep ? cd : +0
//     dp_e = g_e * (dO[i, h, :] . V[j, h, :] chain)     one multiplication
//     p_e, D_i, ds_e = csr5_attention_bwd.hip's with this dp; dQ, dK and dB from ds as csr5_attention_bwd_edge.hip's
//     dV[j, h, :] = sum over the column's entries of fma(p_e * g_e, dO[i, h, :], acc)   (p_e * g_e: one multiplication)
//
// The workspace (M, 1 / Z, D) keeps its meaning.  With p = 0 (g = 1) every bit is csr5hip_mha_edge_bias_backward's.  The same kernel
// templates (csr5_attention_bwd_kern.h) on an argument struct derived from the edge one (AttBwdDropArgs: ARGS::DROP); no other
// instantiation is touched.  THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_attention_bwd_edge.hip
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdDropArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdDropArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdDropArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_drop_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdDropArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdDropArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
