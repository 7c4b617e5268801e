// csr5_attention_bwd_lowp.hip -- csr5hip_mha_lowp_backward: csr5_attention_bwd_edge.hip's call (the gradients of packed multi-head
// attention with a softmax scale and a per-head edge bias for Q, K, V and, on request, the bias tensor B, in TWO launches) on
// operands STORED IN 16 BITS, for gfx950 (wave64):
//
//     Q, K, V, B and dO are bf16 or fp16 (the operand type ST), and dQ, dK, dV and dB are written in it;
//     EVERYTHING COMPUTED IS float, and so is the workspace (4 m heads values: M, 1 / Z, D and one unused per (row, head)).
//
// A bf16 or fp16 number is a float exactly, so the definition is short: the kernels widen an operand where they load it, run
// k_attention_bwd_edge<float, ..>'s statements in their order -- the chains of s and dp, M, w, Z, D and their trees, p, ds,
// t = ds * c, the stage in LDS, the accumulators and their reductions -- and round each output once, to nearest even, where they
// store it.  The line classes, the rank -> storage map, the head groups, the lane <-> column mapping and every summation order are
// functions of (L, width), not of the operand type, so, for each of dQ, dK, dV and dB,
//
//     csr5hip_mha_lowp_backward(Q, K, V, B, dO, scale)
//         == round_ST(csr5hip_mha_edge_bias_backward(float(Q), float(K), float(V), float(B), float(dO), scale))
//
// on an fp32 handle of the same pattern, bit for bit (NaN payloads apart).  The scores are the forward's bits (csr5_attention_lowp.hip),
// and an entry has the same s, p and ds in the row kernel and in the column kernel: the workspace carries M, 1 / Z and D UNROUNDED
// between them, which is why it is float whatever the operand type.  These are the same kernel templates
// (csr5_attention_bwd_kern.h) with an argument struct whose operand and output pointers are ST (AttBwdLowpArgs); no other
// instantiation is touched.
//
// LOADS: both chains (Q . K and dO . V) take their rows by 16-byte loads of 8 elements, in blocks of 32 bytes, under
// attention_bwd_vec's rule in sizeof(ST): Q, K, V and dO 16-byte aligned, their four leading dimensions times 2 multiples of 16
// and, with heads > 1, k * 2 and d * 2 multiples of 16; anything else goes element by element, and a chain runs c = 0, 1, 2, ...
// either way: no bit depends on which.  Operands need 2-byte alignment only.  The accumulations read K, Q and dO element by
// element, one column per lane as in the float kernels, and B one element per (entry, head) -- in the column kernel through the
// companion's source map, a scattered 2-byte read.
// STORES: every store of an output goes through att_stored, which keeps the float value whole in a register before the one
// conversion: the backward ends in p * (dp - D), in the last fma of a chain and in the final adds of a tree, which the compiler
// otherwise folds into the conversion (v_fma_mixlo_f16 and its kin) -- the exact result rounded once to 16 bits instead of the
// float result rounded, another number at a tie.  An fp16 output is +-Inf where the float result exceeds 65 504.
// THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ: the call is the same on an fp32 and on an fp64 handle.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// The product build compiles this file once per operand type (-DCSR5_LOWP_ONLY_BF16 / -DCSR5_LOWP_ONLY_F16), as
// csr5_attention_lowp.hip: each object holds the shared launcher's instantiation on its type, the bf16 one the dispatcher as well.
#if !defined(CSR5_LOWP_ONLY_F16)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpArgs<_Float16>>;
template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpArgs<__bf16>>;
#endif
#if !defined(CSR5_LOWP_ONLY_BF16)
template AttBwdLaunch attention_bwd_launch<float, AttBwdLowpArgs<_Float16>>;
#endif

#if !defined(CSR5_LOWP_ONLY_F16)
// operand_type: CSR5HIP_BF16 or CSR5HIP_F16 (the caller has checked it)
hipError_t launch_mha_lowp_bwd(const Geometry &g, const DeviceArrays &d, int operand_type, const AttBwdCall &c, hipStream_t s)
{
    if (operand_type == CSR5HIP_BF16)
        return attention_bwd_launch<float, AttBwdLowpArgs<__bf16>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdLowpArgs<_Float16>>(g, d, c, s);
}
#endif

} // namespace csr5
