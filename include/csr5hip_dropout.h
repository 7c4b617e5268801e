/* csr5hip_dropout.h -- the part of the C ABI of libcsr5hip.so in which the attention weights are DROPPED OUT: a seeded mask after the
 * softmax and before the product with V, inside csr5hip_mha_edge_bias's and csr5hip_gat's kernels and inside their backwards, with
 * nothing of length nnz written and the handle left alone.  Included by csr5hip.h (inside its extern "C" block, after its types):
 * include that header, not this one. */
#ifndef CSR5HIP_DROPOUT_H
#define CSR5HIP_DROPOUT_H

/* THE MASK.  Philox4x32-10 (multipliers 0xD2511F53 and 0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85).  For the stored entry of
 * CSR rank e IN THE PARENT'S PATTERN (the index B[e, h] uses) and the absolute head g = head0 + h:
 *     counter = (uint32 e, uint32 (g >> 2), offset & 0xFFFFFFFF, offset >> 32)
 *     key     = (seed & 0xFFFFFFFF, seed >> 32)
 *     dropped = philox4x32_10(counter, key)[g & 3] < thr        thr = min(llrint(p * 2^32), 2^32 - 1) as uint32, formed on the host
 *     cd      = (VT)(1.0 / (1.0 - p))                           formed in double, converted once to the handle's type
 * 0 <= p < 1; head0 >= 0 and head0 + heads <= INT_MAX, so that every absolute head is an int.  The mask is a pure function of
 * (p, seed, offset, e, g): the forward and both backward kernels recompute it, a numpy restatement reproduces it bit for bit
 * (tests/dropout_reference.py), and it makes no claim to match any other generator's stream.
 * seed and offset are BY-VALUE ARGUMENTS: a captured call replays the mask it was captured with.  Fresh masks per step are the
 * caller's business (offset = step is the idiom).  p = 0 gives thr = 0 and cd = 1: nothing is dropped, and every output of the four
 * calls below has the bits of the undropped sibling's. */

/* Extension (not in the reference): csr5hip_mha_edge_bias (d_B == NULL: no bias) with dropout on the weights, in ONE launch.  Every
 * argument up to ldo is that call's.  Per row i and head h, every operation rounded once:
 *     M, w_e, Z    = csr5hip_mha_edge_bias's: the softmax is over ALL stored entries of the row, dropped ones included
 *     O[i, h, :]   = (sum over the row's entries of fma(keep_e ? w_e : +0, V[j, h, :], acc)) * (rinv * cd)     rinv = 1 / Z
 * in csr5hip_mha's summation orders; rinv * cd is one multiplication per row and head.  A dropped entry still goes through the FMA, as
 * a -Inf-masked one does.  Head h of a packed call is, bit for bit, the heads = 1 call with head0 + h on that head's slices.
 * THE HANDLE IS UNTOUCHED, nothing is allocated or read back, nothing of length nnz is written; the call only enqueues one kernel on
 * the handle's stream (capturable from the first call on; a replay repeats the mask).
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0, a non-finite
 * scale, p not finite, p < 0, p >= 1, head0 < 0 or head0 + heads > INT_MAX; then as csr5hip_mha_edge_bias from its leading
 * dimensions on.  Single handles only; operands of the handle's type (fp32 or fp64) only. */
int csr5hip_dropout_mha(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo,
                double p, unsigned long long seed, unsigned long long offset, int head0);
/* Extension (not in the reference): the gradients of csr5hip_dropout_mha's O in TWO launches; every argument up to lddb is
 * csr5hip_mha_edge_bias_backward's, (p, seed, offset, head0) the forward's.  Both kernels recompute the mask; the column kernel
 * reaches the entry's rank through the companion's source map, as it reaches B.  Per entry and head, every operation rounded once:
 *     g_e  = keep_e ? cd : +0
 *     dp_e = g_e * (dO[i, h, :] . V[j, h, :] chain)              one multiplication, on both sides
 *     p_e, D_i, ds_e, dQ, dK, dB = csr5hip_mha_edge_bias_backward's with this dp
 *     dV[j, h, :] = sum over the column's entries of fma(p_e * g_e, dO[i, h, :], acc)      p_e * g_e: one multiplication
 * The workspace (M, 1 / Z, D per row and head) keeps its meaning.  Outputs, the companion, d_work, the zeros of nnz = 0, capture and the
 * untouched handle are the sibling's.  Returns as csr5hip_mha_edge_bias_backward, with p not finite, p < 0, p >= 1, head0 < 0 and
 * head0 + heads > INT_MAX added to its first CSR5HIP_INVALID_ARGUMENT group. */
int csr5hip_dropout_mha_backward(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work,
                void *d_dB, int lddb,
                double p, unsigned long long seed, unsigned long long offset, int head0);
/* Extension (not in the reference): csr5hip_gat with the same dropout on the weights, in ONE launch.  The score is csr5hip_gat's, bit
 * for bit; everything after it is csr5hip_dropout_mha's.  Returns as csr5hip_gat with the five mistakes above added to its first group. */
int csr5hip_dropout_gat(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo,
                double p, unsigned long long seed, unsigned long long offset, int head0);
/* Extension (not in the reference): the gradients of csr5hip_dropout_gat's O in TWO launches: csr5hip_gat_backward with g_e, dp_e and
 * dV's coefficient as csr5hip_dropout_mha_backward; dQ, dK and dAr from ds as csr5hip_gat_backward.  Returns as that call with the five
 * mistakes above added to its first group. */
int csr5hip_dropout_gat_backward(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work,
                void *d_dB, int lddb, void *d_dAr, int lddar,
                double p, unsigned long long seed, unsigned long long offset, int head0);
/* Extension (not in the reference): the mask itself, the public way to reproduce it: for every entry e < nnz and head h < heads one
 * byte, 1 kept and 0 dropped, at d_mask[e * ldm + h]; bytes beyond `heads` of a row are not written.  It needs only nnz, so CSR and
 * CSR5 format are served alike.  One launch on the handle's stream; nothing allocated, nothing of the handle read or changed.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, p not finite, p < 0, p >= 1, head0 < 0,
 * head0 + heads > INT_MAX or ldm < heads; CSR5HIP_INVALID_ARGUMENT for a null d_mask with nnz > 0 and heads > 0;
 * CSR5HIP_UNKOWN_FORMAT before input_csr.  heads = 0 or nnz = 0 is then a successful no-op. */
int csr5hip_dropout_mask(csr5hip_handle h, int heads, double p, unsigned long long seed, unsigned long long offset, int head0,
                void *d_mask, int ldm);

#endif /* CSR5HIP_DROPOUT_H */
