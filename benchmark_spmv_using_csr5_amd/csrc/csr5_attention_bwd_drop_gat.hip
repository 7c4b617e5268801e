// csr5_attention_bwd_drop_gat.hip -- csr5hip_dropout_gat_backward: csr5_attention_bwd_gat.hip's gradients under csr5_attention_drop_gat.hip's
// dropout mask, in TWO launches, for gfx950 (wave64).  u, l and s are the forward's bits; g_e, dp_e = g_e * (chain) and dV's coefficient
// p_e * g_e are csr5_attention_bwd_drop.hip's; dQ, dK and dAr are formed from ds as csr5hip_gat_backward forms them.  With p = 0 every
// bit is csr5hip_gat_backward's.  The same kernel templates (csr5_attention_bwd_kern.h) on an argument struct derived from the additive
// one (AttBwdDropGatArgs: ARGS::GAT and ARGS::DROP); no other instantiation is touched.  THE HANDLE'S VALUES ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// once per value type, as csr5_attention_bwd_gat.hip
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdDropGatArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdDropGatArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdDropGatArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_gat_drop_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdDropGatArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdDropGatArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
