// csr5_attention_bwd_drop_lowp.hip -- csr5hip_dropout_mha_lowp_backward: csr5_attention_bwd_drop.hip's call (the gradients of dropped
// packed multi-head attention for Q, K, V and, on request, the bias tensor B, in TWO launches) on operands STORED IN 16 BITS, for
// gfx950 (wave64):
//
//     Q, K, V, B and dO are bf16 or fp16 (the operand type ST), and dQ, dK, dV and dB are written in it;
//     EVERYTHING COMPUTED IS float -- g_e = keep ? cd : +0 with cd = (float)(1 / (1 - p)) included --, and so is the workspace
//     (4 m heads values: M, 1 / Z, D and one unused per (row, head)), which holds the float call's bits.
//
// The kernels widen an operand where they load it (csr5_attention_bwd_lowp.hip), run k_attention_bwd_drop<float, ..>'s statements in
// their order -- dp_e = g_e * (dO . V chain), p, D, ds, t = ds * c, dV's coefficient p_e * g_e -- and round each output once where
// they store it (att_stored).  Both kernels recompute the forward's mask from the entry's rank in the PARENT's CSR order: the
// position walked in the row kernel, the companion's source map word in the column kernel.  So, for each of dQ, dK, dV and dB,
//
//     csr5hip_dropout_mha_lowp_backward(Q, K, V, B, dO, scale, p, seed, offset, head0)
//         == round_ST(csr5hip_dropout_mha_backward(float(Q), float(K), float(V), float(B), float(dO), scale, p, seed, offset, head0))
//
// on an fp32 handle of the same pattern, bit for bit (NaN payloads apart), and with p = 0 every word is csr5hip_mha_lowp_backward's.
// The same kernel templates (csr5_attention_bwd_kern.h) on an argument struct derived from the 16-bit one (AttBwdLowpDropArgs:
// ARGS::DROP); no other instantiation is touched.  The load widths follow csr5_attention_bwd_lowp.hip's rules.
// THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ: the call is the same on an fp32 and on an fp64 handle.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// once per operand type (-DCSR5_LOWP_ONLY_BF16 / -DCSR5_LOWP_ONLY_F16), as csr5_attention_bwd_lowp.hip
#if !defined(CSR5_LOWP_ONLY_F16)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpDropArgs<_Float16>>;
template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpDropArgs<__bf16>>;
#endif
#if !defined(CSR5_LOWP_ONLY_BF16)
template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpDropArgs<_Float16>>;
#endif

#if !defined(CSR5_LOWP_ONLY_F16)
// operand_type: CSR5HIP_BF16 or CSR5HIP_F16 (the caller has checked it)
hipError_t launch_mha_lowp_drop_bwd(const Geometry &g, const DeviceArrays &d, int operand_type, const AttBwdCall &c, hipStream_t s)
{
    if (operand_type == CSR5HIP_BF16)
        return attention_bwd_launch<float, AttBwdLowpDropArgs<__bf16>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdLowpDropArgs<_Float16>>(g, d, c, s);
}
#endif

} // namespace csr5
