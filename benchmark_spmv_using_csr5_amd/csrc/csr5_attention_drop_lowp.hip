// csr5_attention_drop_lowp.hip -- csr5hip_dropout_mha_lowp: csr5_attention_drop.hip's call (packed multi-head attention with a softmax
// scale, a per-head edge bias and a seeded DROPOUT MASK ON THE WEIGHTS, in ONE launch) on operands STORED IN 16 BITS, for gfx950
// (wave64):
//
//     Q, K, V, B and O are bf16 or fp16 (the operand type ST); EVERYTHING COMPUTED IS float, cd = (float)(1 / (1 - p)) included.
//
// The two extensions meet without a new statement: the kernel widens an operand where it loads it (csr5_attention_lowp.hip), runs
// k_attention_drop<float, ..>'s statements in their order -- M, w and Z over ALL stored entries, keep ? w : +0 into the product,
// rinv * cd once per row and head -- and rounds O once, to nearest even, where it stores it.  The mask is csr5hip_dropout.h's: the
// same counter (the entry's CSR rank in the parent's pattern, the absolute head head0 + h), key and thr, so
//
//     csr5hip_dropout_mha_lowp(Q, K, V, B, scale, p, seed, offset, head0)
//         == round_ST(csr5hip_dropout_mha(float(Q), float(K), float(V), float(B), scale, p, seed, offset, head0))
//
// on an fp32 handle of the same pattern, bit for bit (NaN payloads apart), and with p = 0 every word is csr5hip_mha_lowp's.  These are
// the same kernel templates (csr5_attention_kern.h) on an argument struct derived from the 16-bit one (AttLowpDropArgs: ARGS::DROP);
// no other instantiation is touched.  The load widths follow csr5_attention_lowp.hip's rules, and no bit depends on them.
// THE HANDLE'S VALUES ARE NOT READ: the call is the same on an fp32 and on an fp64 handle.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// once per operand type (-DCSR5_LOWP_ONLY_BF16 / -DCSR5_LOWP_ONLY_F16), as csr5_attention_lowp.hip: the bf16 object holds the dispatcher
#if !defined(CSR5_LOWP_ONLY_F16)
extern template AttLaunch attention_launch<AttLowpDropArgs<_Float16>>;
template AttLaunch attention_launch<AttLowpDropArgs<__bf16>>;
#endif
#if !defined(CSR5_LOWP_ONLY_BF16)
template AttLaunch attention_launch<AttLowpDropArgs<_Float16>>;
#endif

#if !defined(CSR5_LOWP_ONLY_F16)
// operand_type: CSR5HIP_BF16 or CSR5HIP_F16 (the caller has checked it)
hipError_t launch_mha_lowp_drop(const Geometry &g, const DeviceArrays &d, int operand_type, const AttCall &c, hipStream_t s)
{
    if (operand_type == CSR5HIP_BF16)
        return attention_launch<AttLowpDropArgs<__bf16>>(g, d, c, s);
    return attention_launch<AttLowpDropArgs<_Float16>>(g, d, c, s);
}
#endif

} // namespace csr5
