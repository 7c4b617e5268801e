/* csr5hip_reduce.h -- the part of the C ABI of libcsr5hip.so that aggregates neighbour rows by the element-wise MAXIMUM or MINIMUM
 * over a row's stored entries (GraphSAGE-pool, PNA's max / min, reduce = "max" of a sparse-dense product), with the argmax and the
 * gradients.  Included by csr5hip.h (inside its extern "C" block, after its types): include that header, not this one.
 *
 * DEFINITION.  t(e, c) = a_e * X[j_e, c] with weighted = 1 and t(e, c) = X[j_e, c] with weighted = 0, for every stored entry e and
 * every c < k.  The product is ONE multiplication, rounded once.  a_e is the handle's CURRENT value of entry e, read from the
 * tile-ordered value array that csr5hip_update_values maintains; with weighted = 0 the handle's values are not read at all.  e is
 * the entry's rank in CSR order: row i holds the ranks row_ptr[i] .. row_ptr[i + 1] - 1, j_e is the column of entry e.
 * ORDER.  For op = CSR5HIP_REDUCE_MAX entry e beats entry f in column c when
 *     t(e, c) is NaN and t(f, c) is not; or
 *     neither is NaN and t(e, c) > t(f, c); or
 *     neither of these decides it, for either of the two, and e < f (equal values, +0 == -0 included, and two NaNs).
 * For op = CSR5HIP_REDUCE_MIN read < for >.  Ranks are distinct, so this is a strict total order: its maximum does not depend on the
 * order or the grouping of the comparisons, and every lane layout computes the same winner.
 * FORWARD.  For every row i and every c < k: arg[i, c] (at d_arg[i * ldarg + c]) is the winning entry's rank as int32, -1 for a row
 * without entries; Y[i, c] (at d_Y[i * ldy + c]) is bit for bit t(arg[i, c], c), +0 for a row without entries.
 *   - Every row of Y and of arg is written for c < k (both may be uninitialised memory); columns k .. ld - 1 are never written.
 *   - NaN propagates and the FIRST NaN wins (torch.amax gives NaN as well).  A row consisting only of -Inf gives -Inf, arg its first
 *     entry.  Repeated (row, column) pairs are separate entries.
 *   - d_arg may be NULL (inference): nothing is written for it.  k = 0 or m = 0 is a successful no-op.
 *   - The bits of a row of Y and of arg depend only on that row's entries, their rows of X, k, op, weighted and the value type: not on
 *     sigma, any option, padding, alignment or the run.
 * BACKWARD.  Given arg from the forward and dY (m x k, lddy):
 *   dX[j, c] = the sum, over the entries e of column j with arg[row(e), c] == e, of a_e * dY[row(e), c] (weighted) or of
 *     dY[row(e), c] (not weighted).  A column kernel on the TRANSPOSED COMPANION's pattern computes it: the entry's rank in A comes
 *     from the companion's source map, a_e from the companion's copy of the values, A's row from the companion's column array.
 *     EVERY row of dX is written for c < k, +0 where nothing wins.  No atomics.  THE SUMMATION TREE IS A FUNCTION OF THE COLUMN'S ENTRY
 *     COUNT L ALONE.  Column j's entries are taken in A's CSR order (positions 0 .. L - 1); the term of a position is the product
 *     above (one multiplication, rounded once) where the entry wins and +0 where it does not; a CHAIN is acc = acc + term from +0
 *     over its positions in ascending order:
 *         L <= 16           one chain over all positions
 *         17 <= L <= 512    four chains, chain q over the positions p with p mod 4 == q:   (c0 + c1) + (c2 + c3)
 *         L > 512           sixteen chains, chain q over the positions p with p mod 16 == q:
 *                           W_w = (c[4w] + c[4w+1]) + (c[4w+2] + c[4w+3]),  w = 0 .. 3;   (W0 + W1) + (W2 + W3)
 *     dX needs csr5hip_build_transpose first; the companion is never built lazily.
 *   dval[e] exists only with weighted = 1: nnz values in CSR order, written by a row kernel on A's own pattern.  It is ONE chain
 *     acc = fma(X[j_e, c], dY[i, c], acc) from +0 over the c with arg[i, c] == e, in ascending c.  An entry that wins nowhere gets +0;
 *     all nnz entries are written.  arg values outside the row's rank range (a corrupt arg) match no entry: nothing is indexed by arg.
 *   Either output may be NULL; a launch whose output is NULL is not made.
 * All three kernels only enqueue on the handle's stream, allocate nothing, read nothing back and change nothing in the handle:
 * csr5hip_info, device_bytes, the values and x stay as they are, and a single-stream graph can capture the calls from the first call
 * on.  Handles of fp64 and fp32; operands of the handle's type; single handles only (no csr5hip_multi).  The mean is csr5hip_spmm
 * followed by one element-wise division by the row length and has no entry point of its own.
 * OUTPUTS MUST NOT OVERLAP INPUTS OR THE HANDLE'S ARRAYS.
 * Returns, decided on the host in this order:
 *   1. CSR5HIP_INVALID_ARGUMENT for a null handle; op or weighted outside {0, 1}; k < 0; a leading dimension below k (ldarg only if
 *      d_arg is given); a null X or Y while there is work (k > 0 and m > 0); backward: a null X while dval is wanted, a null dY or
 *      arg while there is work, or d_dval_csr given with weighted = 0.
 *   2. CSR5HIP_UNSUPPORTED_CSR_SPMV in CSR format, CSR5HIP_UNKOWN_FORMAT before inputCSR (as csr5hip_spmm).
 *   3. CSR5HIP_INVALID_ARGUMENT, csr5hip_last_error() saying "call csr5hip_build_transpose first", when dX is wanted and the handle
 *      has no transposed companion. */
#ifndef CSR5HIP_REDUCE_H
#define CSR5HIP_REDUCE_H

#define CSR5HIP_REDUCE_MAX 0
#define CSR5HIP_REDUCE_MIN 1

int csr5hip_spmm_reduce(csr5hip_handle h, int op, int weighted, const void *d_X, int ldx, int k,
                        void *d_Y, int ldy, int32_t *d_arg, int ldarg);
int csr5hip_spmm_reduce_backward(csr5hip_handle h, int weighted, const void *d_X, int ldx, int k,
                                 const void *d_dY, int lddy, const int32_t *d_arg, int ldarg,
                                 void *d_dX, int lddx, void *d_dval_csr);

#endif /* CSR5HIP_REDUCE_H */
