// csr5_attention_lowp.hip -- csr5hip_mha_lowp: csr5_attention_edge.hip's call (packed multi-head attention with a softmax scale and
// a per-head edge bias from a caller's (nnz, heads) tensor, in ONE launch) on operands STORED IN 16 BITS, for gfx950 (wave64):
//
//     Q, K, V, B and O are bf16 or fp16 (the operand type ST); EVERYTHING COMPUTED IS float.
//
// A bf16 or fp16 number is a float exactly, so the definition is short: the kernel widens an operand where it loads it, runs
// k_attention_edge<float, ..>'s statements in their order -- the chain att_score, s = fma(qk, c, b), M, w, Z and its tree, the
// accumulators, acc * rinv, the stage in LDS -- and rounds O once, to nearest even, where it stores it.  The row classes, the
// rank -> storage map, the head groups, the lane <-> column mapping and every summation order are functions of (L, width), not of
// the operand type, so
//
//     csr5hip_mha_lowp(Q, K, V, B, scale)  ==  round_ST(csr5hip_mha_edge_bias(float(Q), float(K), float(V), float(B), scale))
//
// on an fp32 handle of the same pattern, bit for bit (NaN payloads apart).  These are the same kernel templates
// (csr5_attention_kern.h) with an argument struct whose operand pointers are ST (AttLowpArgs); no other instantiation is touched.
//
// LOADS: the chain takes Q and K by 16-byte loads of 8 elements, in blocks of 32 bytes (16 elements), under attention_vec's rule
// in sizeof(ST): k >= 16, Q and K 16-byte aligned, ld * 2 a multiple of 16 and, with heads > 1, k * 2 a multiple of 16; anything
// else goes element by element, and the chain runs c = 0, 1, 2, ... either way.  Operands need 2-byte alignment only.  V and B are
// read element by element, one column per lane as in the float kernel (two columns per lane would change the slot count and with
// it the summation order).
// CONVERSIONS are the compiler's casts: bf16 -> float a 16-bit shift, fp16 -> float v_cvt_f32_f16, float -> bf16 / fp16 one
// round-to-nearest-even (v_cvt_pk_bf16_f32 / v_cvt_f16_f32).  An fp16 O is +-Inf where the float result exceeds 65 504.
// THE HANDLE'S VALUES ARE NOT READ: the call is the same on an fp32 and on an fp64 handle.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// The product build compiles this file once per operand type (-DCSR5_LOWP_ONLY_BF16 / -DCSR5_LOWP_ONLY_F16), as the other units are
// compiled per value type: each object holds the shared launcher's instantiation on its type, the bf16 one the dispatcher as well.
#if !defined(CSR5_LOWP_ONLY_F16)
extern template AttLaunch attention_launch<AttLowpArgs<_Float16>>;
template AttLaunch attention_launch<AttLowpArgs<__bf16>>;
#endif
#if !defined(CSR5_LOWP_ONLY_BF16)
template AttLaunch attention_launch<AttLowpArgs<_Float16>>;
#endif

#if !defined(CSR5_LOWP_ONLY_F16)
// operand_type: CSR5HIP_BF16 or CSR5HIP_F16 (the caller has checked it)
hipError_t launch_mha_lowp(const Geometry &g, const DeviceArrays &d, int operand_type, const AttCall &c, hipStream_t s)
{
    if (operand_type == CSR5HIP_BF16)
        return attention_launch<AttLowpArgs<__bf16>>(g, d, c, s);
    return attention_launch<AttLowpArgs<_Float16>>(g, d, c, s);
}
#endif

} // namespace csr5
