// csr5_attention_bwd_gat.hip -- csr5hip_gat_backward: the gradients of csr5_attention_gat.hip's O for Q, K, V, on request for the
// bias tensor B, and per row for the attention vector a, in TWO launches, for gfx950 (wave64).  Per stored entry e = (i, j), head h
// and channel c, every operation its own rounding:
//
//     u_ec, l_ec, s_e = the forward's, recomputed: the same bits on the row side and on the column side (Q's element is the
//                       first operand of the addition on both)
//     p_e, dp_e, D_i, ds_e = csr5_attention_bwd.hip's, with these scores
//     t_e  = ds_e * c                                   (one rounded multiplication, as the edge call)
//     g_ec = u_ec > 0 ? 1 : ns        w_ec = a[h, c] * g_ec          (one rounding; a null: w = g)
//     dQ[i, c]  = sum over the row's entries    of fma(t_e, w_ec, acc)      the row kernel
//     dK[j, c]  = sum over the column's entries of fma(t_e, w_ec, acc)      the column kernel, on the companion
//     dAr[i, c] = sum over the row's entries    of fma(t_e, l_ec, acc)      the row kernel: the row's share of a's gradient
//     dV, dB                                            exactly csr5_attention_bwd_edge.hip's
//
// The gradient of a is dAr summed over the rows, which is the caller's reduction: per-row partials keep the kernels free of atomics
// and of a reduction across workgroups.  These are the same kernel templates (csr5_attention_bwd_kern.h) instantiated with an argument
// struct derived from the edge one (AttBwdGatArgs: ARGS::GAT); the accumulations are routines of their own (gat_short_acc,
// gat_wave_acc, gat_hub_acc), which keep bwd_*_acc's orders and compute the operand from one loaded element and the line's own
// row instead of loading it, the row side with a second chain for dAr next to dQ's.  No other instantiation is touched.
// THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ.
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
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdGatArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdGatArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdGatArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_gat_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdGatArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdGatArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
