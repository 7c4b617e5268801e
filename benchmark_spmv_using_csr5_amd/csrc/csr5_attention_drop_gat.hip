// csr5_attention_drop_gat.hip -- csr5hip_dropout_gat: csr5_attention_gat.hip's additive (GAT, GATv2) attention with csr5_attention_drop.hip's
// dropout on the weights, in ONE launch, for gfx950 (wave64).  The score is csr5hip_gat's, bit for bit; everything after it is
// csr5hip_dropout_mha's: M, w and Z over all stored entries, keep ? w : +0 into the product, rinv * cd once per row and head.  With
// p = 0 every bit is csr5hip_gat's.  The same kernel templates (csr5_attention_kern.h) on an argument struct derived from the additive
// one (AttDropGatArgs: ARGS::GAT and ARGS::DROP); no other instantiation is touched.  THE HANDLE'S VALUES ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// once per value type, as csr5_attention_gat.hip
#if !defined(CSR5_ATTENTION_ONLY_F32)
extern template AttLaunch attention_launch<AttDropGatArgs<float>>;
template AttLaunch attention_launch<AttDropGatArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttDropGatArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_gat_drop(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttDropGatArgs<double>>(g, d, c, s);
    return attention_launch<AttDropGatArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
