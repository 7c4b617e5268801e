/* csr5hip_dropout_lowp.h -- the part of the C ABI of libcsr5hip.so in which the DROPPED attention calls take their operands in 16 BITS
 * (bf16 or fp16) and compute in fp32: csr5hip_dropout.h's mask inside csr5hip_lowp.h's kernels.  Included by csr5hip.h (inside its
 * extern "C" block, after its types and after csr5hip_lowp.h, whose operand-type constants it uses): include that header, not this one. */
#ifndef CSR5HIP_DROPOUT_LOWP_H
#define CSR5HIP_DROPOUT_LOWP_H

/* Extension (not in the reference): csr5hip_dropout_mha on operands STORED in bf16 (operand_type CSR5HIP_BF16) or fp16 (CSR5HIP_F16), in
 * ONE launch.  d_Q, d_K, d_V, d_B and d_O hold that type, in csr5hip_mha's packed layout; all leading dimensions count its elements;
 * d_B = NULL is no bias and reads nothing.  EVERYTHING COMPUTED IS fp32, by csr5hip_dropout_mha's definition on an fp32 handle: an
 * operand is widened where it is loaded, which is exact; c is `scale` converted once to float; cd = (float)(1.0 / (1.0 - p)); the
 * softmax is over ALL stored entries; O is rounded ONCE, to nearest even, where it is stored.  THE MASK IS csr5hip_dropout.h's: the
 * same counter (the entry's CSR rank in the parent's pattern, the absolute head head0 + h), the same key and the same thr, so
 * csr5hip_dropout_mask's bytes describe it.  On an fp32 handle of the same pattern, bit for bit (NaN payloads are not specified):
 *     csr5hip_dropout_mha_lowp(Q, K, V, B, scale, p, seed, offset, head0)
 *         ==  round(csr5hip_dropout_mha(float(Q), float(K), float(V), float(B), scale, p, seed, offset, head0))
 * With p = 0 every word is csr5hip_mha_lowp's.  Head h of a packed call is the heads = 1 call with head0 + h on that head's slices.
 * 16-BYTE LOADS by csr5hip_mha_lowp's rule; no bit depends on them.  THE HANDLE'S VALUES ARE NOT READ: the same words on an fp32 and on
 * an fp64 handle.  The call enqueues one kernel on the handle's stream, allocates nothing, reads nothing back (capturable from the
 * first call on; a replay repeats the mask) and leaves the handle untouched.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle; CSR5HIP_UNSUPPORTED_VALUE_TYPE for an
 * operand type other than the two; then exactly csr5hip_dropout_mha's list from heads < 0 on (p and head0 are judged in that first
 * group, before the leading dimensions).  Single handles only. */
int csr5hip_dropout_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d, void *d_O, int ldo,
        double p, unsigned long long seed, unsigned long long offset, int head0);
/* Extension (not in the reference): its gradients, csr5hip_dropout_mha_backward on operands STORED in 16 bits, in TWO launches.  d_Q,
 * d_K, d_V, d_B and d_dO hold `operand_type`, and d_dQ, d_dK, d_dV and d_dB are written in it; all leading dimensions count its
 * elements.  d_work is FLOAT, 4 * m * heads values, whatever the handle's value type, and holds the fp32 call's bits (M, 1 / Z, D per
 * row and head, unrounded).  EVERYTHING COMPUTED IS fp32 -- g_e = keep_e ? cd : +0 with the float cd included --, both kernels
 * recompute the forward's mask (the column kernel reaches the entry's rank through the companion's source map), and for each of dQ,
 * dK, dV and dB, on an fp32 handle of the same pattern, bit for bit (NaN payloads are not specified):
 *     csr5hip_dropout_mha_lowp_backward(Q, K, V, dO, B, scale, p, seed, offset, head0)
 *         ==  round(csr5hip_dropout_mha_backward(float(Q), float(K), float(V), float(dO), float(B), scale, p, seed, offset, head0))
 * each output rounded ONCE, to nearest even, where it is stored.  With p = 0 every word is csr5hip_mha_lowp_backward's.
 * Everything else is csr5hip_mha_lowp_backward's contract: any output may be NULL; dK and dV need the transposed companion
 * (csr5hip_build_transpose, never built lazily) and d_work, dQ and dB neither; every element of a wanted output is written, the zeros
 * of a pattern without entries in 2-byte elements; the call is enqueue-only, allocates nothing, and is capturable from its first call
 * once the companion exists.  THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle; CSR5HIP_UNSUPPORTED_VALUE_TYPE for an
 * operand type other than the two; then exactly csr5hip_dropout_mha_backward's list from heads < 0 on, the missing-companion message
 * under this call's name.  Single handles only. */
int csr5hip_dropout_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
        const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
        void *d_work, void *d_dB, int lddb,
        double p, unsigned long long seed, unsigned long long offset, int head0);

#endif /* CSR5HIP_DROPOUT_LOWP_H */
