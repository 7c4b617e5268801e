/* csr5hip_edge_bias.h -- the part of the C ABI of libcsr5hip.so in which attention takes a PER-HEAD EDGE BIAS from a caller-owned
 * tensor: a softmax scale and an additive score bias B (nnz x heads) on csr5hip_mha's packed layout, with the handle left alone.
 * Included by csr5hip.h (inside its extern "C" block, after its types): include that header, not this one. */
#ifndef CSR5HIP_EDGE_BIAS_H
#define CSR5HIP_EDGE_BIAS_H

/* Extension (not in the reference): csr5hip_mha with a softmax scale and an additive score bias that differs per entry AND per head,
 * softmax(scale * Q K^T + B) V on the pattern, in ONE launch on csr5hip_mha's packed layout: the learned edge bias of a graph
 * transformer (B = Linear(edge_attr)), which changes every step and which csr5hip_mha_biased (one stored value per entry, a slope
 * per head) can only give head by head through csr5hip_update_values.
 * d_B holds nnz x heads values of the handle's type: element (e, h) at B[e * ldb + h], ldb >= heads; e is the entry's CSR RANK, the
 * order csr5hip_sddmm writes and csr5hip_update_values takes; repeated (row, column) pairs are separate entries with their own
 * bias.  d_B is read only and never retained; columns heads .. ldb - 1 of a row of B are never read.  d_B == NULL means no bias:
 * b = +0 and nothing is read for it -- scaled attention that does not read the handle's values.
 * SCORE, per stored entry e and head h, every operation rounded once (fp contract(off), the FMAs written out):
 *     qk_e,h = csr5hip_sddmm's chain on head h's slices of Q and K, unchanged
 *     s_e,h  = fma(qk_e,h, c, B[e, h]), c = `scale` converted once to the handle's type
 * EVERYTHING AFTER THE SCORE IS csr5hip_mha's, per head, with these scores: M, w, Z and its tree, the normalisation after the
 * product, the summation orders as a function of (L, width), the row classes, +0 for rows without entries, the head groups, the
 * 16-byte-load rule and the determinism contract (to which the row's biases and c are added).
 * THE HANDLE IS UNTOUCHED: its values (the parent's and the companion's), x, the options, csr5hip_info and device_bytes are neither
 * read nor written; nothing is allocated or read back; the call only enqueues one kernel on the handle's stream (capturable from
 * the first call on).
 * NON-FINITE: a -Inf bias has weight +0: a hard mask of that entry in that head.  A row that in some head holds a NaN score, holds
 * a +Inf score or consists only of -Inf scores is NaN in that head's outputs; no other row and no other head is affected.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0 or a non-finite
 * scale; CSR5HIP_INVALID_ARGUMENT for a leading dimension below heads times its width or, with d_B given, ldb < heads (compared in
 * 64 bits); then as csr5hip_mha from its null operands on.  heads = 0, d = 0 or m = 0 is then a successful no-op.  Single handles
 * only. */
int csr5hip_mha_edge_bias(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo);
/* Extension (not in the reference): the gradients of csr5hip_mha_edge_bias's O in TWO launches; Q, K, V, dO, dQ, dK, dV and d_work
 * exactly as csr5hip_mha_backward, d_B / ldb as above.  p, dp, D and ds are csr5hip_attention_backward's with the scores s_e,h
 * above (the same bits as the forward's, on the row side and on the column side); then
 *     t_e = ds_e * c, ONE rounded multiplication;  dQ = sum_e t_e K[j_e],  dK = sum_e t_e Q[i_e]  by csr5hip_mha_backward's
 *     accumulation rules;  dV is unchanged (sum_e p_e dO[i_e]).
 * d_dB (optional, NULL: not wanted): dB[e * lddb + h] = ds_e,h, nnz x heads values of the handle's type, e in CSR order,
 * lddb >= heads: THE GRADIENT OF B, no reduction is needed.  Every (entry, head) is written and nothing beyond column heads - 1 of
 * a row of dB; the row kernel writes it, exactly as csr5hip_mha_biased_backward writes dS.
 * The row kernel reads B at the entry's CSR rank; the column kernel walks the TRANSPOSED COMPANION's pattern and finds the entry's
 * rank through the companion's source map, so an entry has the same s, p and ds on both sides.  Neither reads the handle's or the
 * companion's values.  Any output may be NULL; every row of a wanted output is fully written and nothing beyond it.  dK or dV
 * requires the companion (never built lazily) and d_work (4 m heads values); dQ and / or dB need neither.  Allocates nothing,
 * reads nothing back, only enqueues (capturable), leaves the handle untouched.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0 or a non-finite scale;
 * CSR5HIP_INVALID_ARGUMENT for a leading dimension below heads times its width, with d_B given ldb < heads or with d_dB given
 * lddb < heads; then as csr5hip_mha_backward from its null operands on (d_dB counts as a wanted output).  All of dQ, dK, dV and dB
 * null, or heads = 0, is then a successful no-op; nnz = 0 only writes the zeros. */
int csr5hip_mha_edge_bias_backward(csr5hip_handle h, int heads, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work,
                void *d_dB, int lddb);

#endif /* CSR5HIP_EDGE_BIAS_H */
