/* csr5hip_lowp.h -- the part of the C ABI of libcsr5hip.so in which attention takes its operands in 16 BITS (bf16 or fp16) and
 * computes in fp32.  Included by csr5hip.h (inside its extern "C" block, after its types): include that header, not this one. */
#ifndef CSR5HIP_LOWP_H
#define CSR5HIP_LOWP_H

#define CSR5HIP_BF16 2   /* operand types of csr5hip_mha_lowp; not handle value types */
#define CSR5HIP_F16  3

/* Extension (not in the reference): csr5hip_mha_edge_bias on operands STORED in bf16 (operand_type CSR5HIP_BF16) or fp16
 * (CSR5HIP_F16): d_Q, d_K, d_V, d_B and d_O all hold that type, in csr5hip_mha's packed layout; all leading dimensions count
 * elements of it.  d_B is nnz x heads in CSR order, element (e, h) at B[e * ldb + h]; NULL means no bias and reads nothing (scaled
 * attention; with scale = 1, csr5hip_mha).  EVERYTHING COMPUTED IS fp32, by csr5hip_mha_edge_bias's definition on an fp32 handle:
 * an operand is widened where it is loaded, which is exact, c is `scale` converted once to float, and O is rounded ONCE, to nearest
 * even, where it is stored.  The row classes, the summation orders, the head groups and the rank -> storage map are functions of
 * (L, width) as there, so
 *     csr5hip_mha_lowp(Q, K, V, B)  ==  round(csr5hip_mha_edge_bias(float(Q), float(K), float(V), float(B)))
 * bit for bit (NaN payloads are not specified).  An fp16 O is +-Inf where the fp32 result exceeds 65 504.
 * 16-BYTE LOADS of 8 elements for Q and K when k >= 16, d_Q and d_K are 16-byte aligned, ldq * 2 and ldk * 2 are multiples of 16 and,
 * with heads > 1, k * 2 is one; element loads otherwise; no bit depends on which.  Operands need 2-byte alignment only.
 * THE HANDLE'S VALUES ARE NOT READ: only the pattern is, and the call gives the same bits on an fp32 and on an fp64 handle.  It
 * enqueues one kernel on the handle's stream, allocates nothing, reads nothing back (capturable from the first call on) and
 * leaves the handle untouched.  Every row and head of O is written, a row without entries with +0.  Non-finite scores behave as in
 * csr5hip_mha_edge_bias.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle; CSR5HIP_UNSUPPORTED_VALUE_TYPE for an
 * operand type other than the two; then exactly csr5hip_mha_edge_bias's list from heads < 0 on.  Single handles only. */
int csr5hip_mha_lowp(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo);

/* Extension (not in the reference): its gradients, csr5hip_mha_edge_bias_backward on operands STORED in 16 bits, in two launches.
 * d_Q, d_K, d_V, d_B and d_dO hold `operand_type`, and d_dQ, d_dK, d_dV and d_dB are written in it; all leading dimensions count its
 * elements.  d_work is FLOAT, 4 * m * heads values, whatever the handle's value type: the column kernel reads back the row kernel's
 * M, 1 / Z and D unrounded.  EVERYTHING COMPUTED IS fp32, and for each of dQ, dK, dV and dB
 *     csr5hip_mha_lowp_backward(Q, K, V, B, dO)
 *         ==  round(csr5hip_mha_edge_bias_backward(float(Q), float(K), float(V), float(B), float(dO)))
 * on an fp32 handle of the same pattern, bit for bit (NaN payloads are not specified): each output is rounded ONCE, to nearest even,
 * where it is stored.  The scores are csr5hip_mha_lowp's bits, and an entry has the same s, p and ds in both kernels.
 * Everything else is csr5hip_mha_edge_bias_backward's contract: any output may be NULL; dK and dV need the transposed companion
 * (csr5hip_build_transpose, never built lazily) and d_work, dQ and dB neither; d_B = NULL is scaled attention and reads nothing;
 * every element of a wanted output is written; the call is enqueue-only, allocates nothing, and is capturable from its first call
 * once the companion exists.  THE HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ: the same bits on an fp32 and on
 * an fp64 handle.
 * 16-BYTE LOADS of 8 elements for the chains Q . K and dO . V when d_Q, d_K, d_V and d_dO are 16-byte aligned, ldq, ldk, ldv and lddo
 * times 2 are multiples of 16 and, with heads > 1, k * 2 and d * 2 are; element loads otherwise; no bit depends on which.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle; CSR5HIP_UNSUPPORTED_VALUE_TYPE for an
 * operand type other than the two; then exactly csr5hip_mha_edge_bias_backward's list from heads < 0 on, the missing-companion
 * message under this call's name.  Single handles only. */
int csr5hip_mha_lowp_backward(csr5hip_handle h, int operand_type, int heads, double scale, const void *d_B, int ldb,
        const void *d_Q, int ldq, const void *d_K, int ldk, int k, const void *d_V, int ldv, int d,
        const void *d_dO, int lddo, void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv,
        void *d_work, void *d_dB, int lddb);

#endif /* CSR5HIP_LOWP_H */
