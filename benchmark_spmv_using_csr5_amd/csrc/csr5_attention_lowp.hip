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

// groups: the head groups over grid.y, 0 for the rule (att_heads_per_group)
template <typename ST>
static hipError_t attention_lowp_typed(const Geometry &g, const DeviceArrays &d, int heads, int groups, double scale, const void *B,
                                       int ldb, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,
                                       void *O, int ldo, hipStream_t s)
{
    static_assert(sizeof(ST) == 2, "a 16-bit operand type");
    if (g.m <= 0 || dcols <= 0 || heads <= 0)
        return hipSuccess;
    AttLowpArgs<ST> A;
    attention_fill<ST>(A, g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo);
    A.bias.B = (const ST *)B;
    A.bias.ldb = ldb;
    A.bias.c = (float)scale;
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    const dim3 grid(blocks, (unsigned)((heads + A.hper - 1) / A.hper)), block(AT_BLOCK);
    if (attention_vec<ST>(heads, Q, ldq, K, ldk, k))
        hipLaunchKernelGGL((k_attention_lowp<ST, true>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((k_attention_lowp<ST, false>), grid, block, 0, s, A);
    return hipGetLastError();
}

// The product build compiles this file once per operand type (-DCSR5_LOWP_ONLY_BF16 / -DCSR5_LOWP_ONLY_F16), as the other units
// are compiled per value type.
#define CSR5_LOWP_PARAMS                                                                                                                  \
    const Geometry &g, const DeviceArrays &d, int heads, int groups, double scale, const void *B, int ldb, const void *Q, int ldq,        \
        const void *K, int ldk, int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s
#define CSR5_LOWP_ARGS g, d, heads, groups, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s
#if !defined(CSR5_LOWP_ONLY_F16)
hipError_t launch_mha_lowp_bf16(CSR5_LOWP_PARAMS) { return attention_lowp_typed<__bf16>(CSR5_LOWP_ARGS); }
#endif
#if !defined(CSR5_LOWP_ONLY_BF16)
hipError_t launch_mha_lowp_f16(CSR5_LOWP_PARAMS) { return attention_lowp_typed<_Float16>(CSR5_LOWP_ARGS); }
#endif

#if !defined(CSR5_LOWP_ONLY_F16)
hipError_t launch_mha_lowp_f16(CSR5_LOWP_PARAMS);

// operand_type: CSR5HIP_BF16 or CSR5HIP_F16 (the caller has checked it)
hipError_t launch_mha_lowp(const Geometry &g, const DeviceArrays &d, int operand_type, int heads, int groups, double scale, const void *B,
                           int ldb, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, void *O,
                           int ldo, hipStream_t s)
{
    return operand_type == CSR5HIP_BF16 ? launch_mha_lowp_bf16(CSR5_LOWP_ARGS) : launch_mha_lowp_f16(CSR5_LOWP_ARGS);
}
#endif
#undef CSR5_LOWP_PARAMS
#undef CSR5_LOWP_ARGS

} // namespace csr5
