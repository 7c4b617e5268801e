// csr5_attention_bwd_bias.hip -- csr5hip_mha_biased_backward: the gradients of csr5_attention_bias.hip's O for Q, K and V, and on
// request for the biased score itself, in TWO launches, for gfx950 (wave64).  Per stored entry e = (i, j) and head h, every
// operation its own rounding:
//
//     s_e  = fma(qk_e, c, b_e), the forward's biased score, the same bits (csr5_attention_bias.hip)
//     p_e, dp_e, D_i, ds_e = csr5_attention_bwd.hip's, with these scores
//     t_e  = ds_e * c                                   (one rounded multiplication)
//     dQ[i, c] = sum_e t_e K[j_e, c]      dK[j, c] = sum_e t_e Q[i_e, c]      dV[j, c] = sum_e p_e dO[i_e, c]
//     dS[e * ldds + h] = ds_e,h           (optional; e the entry's CSR rank: the gradient for the biased score, before c and slope)
//
// by csr5_attention_bwd.hip's accumulation rules, row classes, workspace and determinism contract: these are the same kernel
// templates (csr5_attention_bwd_kern.h) instantiated with an argument struct that carries the bias (AttBwdBiasArgs); the plain
// instantiations are not touched by it.  THE ROW KERNEL reads the parent's values and writes dS (every (entry, head), a head
// group its own heads' elements, nothing beyond column heads - 1 of a row of dS); THE COLUMN KERNEL reads the transposed
// companion's values at the companion's storage position, so an entry has the same s, p and ds on both sides.  A row beyond
// 2 048 entries, whose ds exists only inside dQ's chunk refills, writes dS in one more sweep of the same recomputation.  The
// values are read, as in the forward, next to the column (kept across the heads by a lane of a short line, read again by every
// head otherwise), and never written.
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
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdBiasArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdBiasArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdBiasArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_biased_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdBiasArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdBiasArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
