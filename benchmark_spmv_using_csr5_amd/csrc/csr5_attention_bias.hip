// csr5_attention_bias.hip -- csr5hip_mha_biased: csr5_attention.hip's packed multi-head attention with a softmax scale and an
// additive score bias taken from the handle's stored values, in ONE launch, for gfx950 (wave64):
//
//     s_e,h = fma(qk_e,h, c, b_e,h)     qk_e,h: csr5_attention.hip's chain on head h's slices, the same bits
//                                       c: the scale, converted once to the value type
//                                       b_e,h = slopes[h] * a_e (one rounded multiplication), or a_e without slopes
//                                       a_e: the handle's value of entry e
//
// and EVERYTHING after the score is csr5_attention.hip's, per head, with these scores: M, w, Z and its tree, the normalisation
// after the product, the summation orders as a function of (L, width), the row classes, +0 for rows without entries, the head
// groups, the 16-byte-load rule and the determinism contract.  These are the same kernel templates (csr5_attention_kern.h)
// instantiated with an argument struct that carries the bias (AttBiasArgs); the plain instantiations are not touched by it.
//
// THE VALUE of an entry is read from the handle's tile-ordered value array at the storage position its column is read from
// (att_storage): once per entry for a row of at most 16 entries, where a lane keeps it across the heads of the workgroup; in the
// longer rows, whose columns are staged in LDS for the later heads, every head reads it again from that position -- staging it
// would take 8 (fp32) or 16 KiB (fp64) more LDS per workgroup.  The values are read and never written.  The bias enters at every
// place a score is computed, the maximum sweep and every chunk refill of a row beyond 2 048 entries included.
//
// NON-FINITE: a -Inf bias gives a -Inf score, weight +0: a hard mask.  A row that holds a NaN score, holds a +Inf score or
// consists only of -Inf scores is NaN in all its outputs, and no other row is affected, as in csr5_attention.hip.
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
extern template AttLaunch attention_launch<AttBiasArgs<float>>;
template AttLaunch attention_launch<AttBiasArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttBiasArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_biased(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttBiasArgs<double>>(g, d, c, s);
    return attention_launch<AttBiasArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
