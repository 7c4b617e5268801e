/* csr5hip_bias.h -- the part of the C ABI of libcsr5hip.so in which the matrix VALUES take part in attention: a softmax scale and an
 * additive score bias on csr5hip_mha's packed layout.  Included by csr5hip.h (inside its extern "C" block, after its types): include
 * that header, not this one. */
#ifndef CSR5HIP_BIAS_H
#define CSR5HIP_BIAS_H

/* Extension (not in the reference): csr5hip_mha with a softmax scale and an additive score bias taken from the handle's STORED
 * VALUES, softmax(scale * Q K^T + slope_h * A) V on the pattern, in ONE launch on csr5hip_mha's packed layout.  This is the one
 * attention call in which the matrix values take part: edge features, a relative-position or distance bias, ALiBi with a slope
 * per head, or a soft or hard (-Inf) mask.
 * SCORE, per stored entry e and head h, every operation rounded separately (fp contract(off), the FMAs written out):
 *     qk_e,h = csr5hip_sddmm's chain on head h's slices of Q and K, unchanged
 *     a_e    = the handle's stored value of entry e -- what csr5hip_input_csr gave or the last csr5hip_update_values
 *     b_e,h  = slopes[h] * a_e, ONE rounded multiplication; d_slopes == NULL: b_e,h = a_e, no multiplication.  d_slopes holds
 *              `heads` device values of the handle's type
 *     s_e,h  = fma(qk_e,h, c, b_e,h), c = `scale` converted once to the handle's type
 * EVERYTHING AFTER THE SCORE IS csr5hip_mha's, per head, with these scores: M, w, Z and its tree, the normalisation after the
 * product, the summation orders as a function of (L, width), the row classes, +0 for rows without entries, the head groups, the
 * 16-byte-load rule and the determinism contract (to which the row's values and the head's slope and c are added).
 * The value is read from the handle's own tile-ordered value array at the storage position the entry's column is read from; the
 * values are READ AND NEVER WRITTEN.  x, the options, csr5hip_info and device_bytes are untouched; nothing is allocated or read
 * back; the call only enqueues one kernel on the handle's stream (capturable).
 * NON-FINITE: a -Inf bias has weight +0: a hard mask.  A row that holds a NaN score, holds a +Inf score or consists only of -Inf
 * scores is NaN in all its outputs, exactly as in csr5hip_attention; no other row is affected.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0 or a non-finite
 * scale; then as csr5hip_mha from its leading dimensions on.  heads = 0, d = 0 or m = 0 is then a successful no-op.  Single
 * handles only. */
int csr5hip_mha_biased(csr5hip_handle h, int heads, double scale, const void *d_slopes,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo);
/* Extension (not in the reference): the gradients of csr5hip_mha_biased's O in TWO launches; Q, K, V, dO, dQ, dK, dV and d_work
 * exactly as csr5hip_mha_backward.  p, dp, D and ds are csr5hip_attention_backward's with the biased scores s_e,h above (the same
 * bits as the forward's, on the row side and on the column side); then
 *     t_e = ds_e * c, ONE rounded multiplication;  dQ = sum_e t_e K[j_e],  dK = sum_e t_e Q[i_e]  by csr5hip_mha_backward's
 *     accumulation rules;  dV is unchanged (sum_e p_e dO[i_e]).
 * d_dS (optional, NULL: not wanted): dS[e * ldds + h] = ds_e,h, the gradient for the biased SCORE, before c and before the slope:
 * nnz x heads values of the handle's type, e in CSR order (the order of csr5hip_update_values), ldds >= heads.  Every (entry,
 * head) is written and nothing beyond column heads - 1 of a row of dS; the row kernel writes it, a head group its own heads'
 * elements.  It is the one nnz-long array this call may write, and only when asked.  The caller forms the gradient of the values,
 * sum_h slopes[h] dS[e, h], and of the slopes, sum_e a_e dS[e, h].
 * The row kernel reads the handle's values, the column kernel the TRANSPOSED COMPANION's (kept current by
 * csr5hip_update_values); neither writes them.  dK or dV requires the companion (never built lazily) and d_work; d_dS together with
 * dQ needs neither.  Allocates nothing, reads nothing back, only enqueues (capturable), leaves the handle untouched.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0 or a non-finite scale;
 * CSR5HIP_INVALID_ARGUMENT for a leading dimension below heads times its width or, with d_dS given, ldds < heads; then as
 * csr5hip_mha_backward from its null operands on (d_dS counts as a wanted output).  All of dQ, dK, dV and dS null, or heads = 0, is
 * then a successful no-op; nnz = 0 only writes the zeros. */
int csr5hip_mha_biased_backward(csr5hip_handle h, int heads, double scale, const void *d_slopes,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work,
                void *d_dS, int ldds);

#endif /* CSR5HIP_BIAS_H */
