/* csr5hip_gat.h -- the part of the C ABI of libcsr5hip.so in which attention scores an entry ADDITIVELY, with the non-linearity inside
 * the score: GAT's LeakyReLU(el[i] + er[j]) and GATv2's a^T LeakyReLU(x_i + x_j), on csr5hip_mha's packed layout, with the handle left
 * alone.  Included by csr5hip.h (inside its extern "C" block, after its types): include that header, not this one. */
#ifndef CSR5HIP_GAT_H
#define CSR5HIP_GAT_H

/* Extension (not in the reference): additive attention on the pattern in ONE launch.  Q (m x heads k), K (n x heads k), V (n x heads d)
 * and O (m x heads d) are csr5hip_mha's packed operands; d_B / ldb, `scale` are csr5hip_mha_edge_bias's (d_B == NULL: b = +0, nothing
 * read).  d_a holds heads x k CONTIGUOUS values of the handle's type, a[h * k + c], the attention vector of head h; d_a == NULL means
 * a = 1 and nothing is read for it.  negative_slope is the slope of the LeakyReLU for u <= 0.
 * SCORE, per stored entry e = (i, j), head h and channel c < k, every operation rounded once (fp contract(off), the FMAs written out):
 *     u_c   = Q[i, h, c] + K[j, h, c]
 *     l_c   = u_c > 0 ? u_c : ns * u_c                  ns = negative_slope converted once to the handle's type
 *     z     = fma(a[h, c], l_c, z), c = 0, 1, 2, ...    z starts at +0; d_a == NULL: fma(1, l_c, z), the bits of z + l_c
 *     s_e,h = fma(z, c, B[e, h])                        c = `scale` converted once to the handle's type
 * GAT is k = 1 with d_a == NULL: s = LeakyReLU(el[i, h] + er[j, h]) with Q = el, K = er.  GATv2 is k = the feature width with d_a.
 * k = 0 is legal: z = +0, the call is csr5hip_mha_edge_bias with k = 0.
 * EVERYTHING AFTER THE SCORE IS csr5hip_mha's, per head, with these scores: M, w, Z and its tree, the normalisation after the product,
 * the summation orders as a function of (L, width), the row classes, +0 for rows without entries, the head groups and the determinism
 * contract, to which a, ns, c and the row's biases are added: head h of a packed call is, bit for bit, the heads = 1 call on that
 * head's slices.  Q and K are read by element loads; no bit depends on an alignment.
 * THE HANDLE IS UNTOUCHED: its values (the parent's and the companion's), x, the options, csr5hip_info and device_bytes are neither
 * read nor written; nothing is allocated or read back; nothing of length nnz is written; the call only enqueues one kernel on the
 * handle's stream (capturable from the first call on).
 * NON-FINITE: a NaN u_c fails u_c > 0 and stays a NaN; a -Inf bias has weight +0, a hard mask of that entry in that head.  A row that
 * in some head holds a NaN score, holds a +Inf score or consists only of -Inf scores is NaN in that head's outputs; no other row and
 * no other head is affected.
 * Returns, decided on the host in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0, a non-finite scale
 * or a non-finite negative_slope; CSR5HIP_INVALID_ARGUMENT for a leading dimension below heads times its width or, with d_B given,
 * ldb < heads (compared in 64 bits); then as csr5hip_mha from its null operands on.  heads = 0, d = 0 or m = 0 is then a successful
 * no-op.  Single handles only; operands of the handle's type (fp32 or fp64) only. */
int csr5hip_gat(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, void *d_O, int ldo);
/* Extension (not in the reference): the gradients of csr5hip_gat's O in TWO launches; Q, K, V, dO, dQ, dK, dV, d_work, d_B / ldb and
 * d_dB / lddb exactly as csr5hip_mha_edge_bias_backward, d_a and negative_slope as above.  p, dp, D and ds are
 * csr5hip_attention_backward's with the scores s_e,h above; u and l are recomputed and are the forward's bits on the row side and on
 * the column side.  Then, every operation rounded once:
 *     t_e  = ds_e * c
 *     g_ec = u_ec > 0 ? 1 : ns        w_ec = a[h, c] * g_ec        (d_a == NULL: w = g)
 *     dQ[i, h, c]  = sum over the row's entries    of fma(t_e, w_ec, acc)     the row kernel
 *     dK[j, h, c]  = sum over the column's entries of fma(t_e, w_ec, acc)     the column kernel, on the transposed companion
 *     dAr[i, h, c] = sum over the row's entries    of fma(t_e, l_ec, acc)     the row kernel
 * by csr5hip_mha_backward's accumulation rules (the order as a function of the line's length and of k); dV and dB are exactly
 * csr5hip_mha_edge_bias_backward's.
 * d_dAr (optional, NULL: not wanted): m x heads k values of the handle's type, element (i, h, c) at dAr[i * lddar + h * k + c],
 * lddar >= heads k: THE ROW'S SHARE of the gradient of a.  The gradient of a[h, c] is the sum of dAr[i, h, c] over the rows i, which
 * is left to the caller (one column reduction): per-row partials keep the kernels free of atomics and deterministic.  It costs one
 * more write as large as dQ's.
 * Any output may be NULL; every row of a wanted output is fully written and nothing beyond it.  dK or dV requires the companion (never
 * built lazily) and d_work (4 m heads values); dQ, dAr and dB need neither.  Allocates nothing, reads nothing back, only enqueues
 * (capturable), leaves the handle untouched; nothing of length nnz is written unless d_dB is given.
 * Returns, in this order: CSR5HIP_INVALID_ARGUMENT for a null handle, heads < 0, k < 0, d < 0, a non-finite scale or a non-finite
 * negative_slope; CSR5HIP_INVALID_ARGUMENT for a leading dimension below heads times its width, with d_B given ldb < heads, with d_dB
 * given lddb < heads or with d_dAr given lddar < heads k; then as csr5hip_mha_backward from its null operands on (d_dB and d_dAr count
 * as wanted outputs, d_dAr as a row-side one).  All of dQ, dK, dV, dB and dAr null, or heads = 0, is then a successful no-op; nnz = 0
 * only writes the zeros (dAr's as dQ's). */
int csr5hip_gat_backward(csr5hip_handle h, int heads, double negative_slope, const void *d_a, double scale, const void *d_B, int ldb,
                const void *d_Q, int ldq, const void *d_K, int ldk, int k,
                const void *d_V, int ldv, int d, const void *d_dO, int lddo,
                void *d_dQ, int lddq, void *d_dK, int lddk, void *d_dV, int lddv, void *d_work,
                void *d_dB, int lddb, void *d_dAr, int lddar);

#endif /* CSR5HIP_GAT_H */
