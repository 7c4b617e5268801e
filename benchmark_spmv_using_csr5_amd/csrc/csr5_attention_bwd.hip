// csr5_attention_bwd.hip -- the gradients of csr5_attention.hip's O for Q, K and V in TWO launches, for gfx950 (wave64), with
// nothing of length nnz written or read back and the handle's values untouched.  dO is the gradient arriving for O (m x d).
//
// DEFINITION per stored entry e = (i, j), every operation its own rounding (fp contract(off), the FMAs written out):
//     s_e  = the forward's chain fma(Q[i, k-1], K[j, k-1], ... fma(Q[i, 0], K[j, 0], +0) ...), the same bits
//     M_i  = the exact maximum of row i's scores,  w_e = exp(s_e - M_i),  Z_i = sum of the row's w by the forward's tree
//     r_i  = 1 / Z_i,  p_e = w_e * r_i                                           (csr5hip_row_softmax's bits)
//     dp_e = fma(dO[i, d-1], V[j, d-1], ... fma(dO[i, 0], V[j, 0], +0) ...)     (csr5hip_sddmm's chain)
//     D_i  = sum over the row of round(p_e * dp_e) by Z's tree,  ds_e = p_e * (dp_e - D_i)   (csr5hip_row_softmax_grad's bits)
//     dQ[i, c] = sum_e ds_e K[j_e, c]       dK[j, c] = sum_e ds_e Q[i_e, c]       dV[j, c] = sum_e p_e dO[i_e, c]
//
// THE ROW KERNEL walks the parent's pattern (row_ptr, tile_ptr, tile-ordered column_index) with the forward's row classes: it
// computes M, r and D of every row, writes them to the workspace (4 values per row: M, r, D, one unused) when one is given, and
// writes dQ when it is wanted.  THE COLUMN KERNEL walks the transposed companion's pattern -- row j of A^T lists the rows i_e of
// the entries of column j in A's CSR order --, with the same classes decided by the column's length: per entry it gathers M, r
// and D of row i_e, recomputes s_e and dp_e by the chains above and p_e and ds_e by the formulas above -- so an entry has the
// same p and ds on both sides --, and writes dV and dK.  No floating-point atomics, no scratch; each kernel reads row_ptr,
// tile_ptr and column_index of its handle and nothing else of it.
//
// EVERY row of a wanted output is written in its k (d) columns, a row (column) of the matrix without entries with +0; nothing is
// written beyond.  A row beyond 2 048 entries recomputes its scores per sweep, as the forward does.
//
// THE SUMMATION ORDER.  Z and D: the forward's Z (csr5_attention.hip), a function of the row's length.  Every accumulation is
// the forward's acc_c rule as a function of (L, width) alone: dQ with (row length, k), dK with (column length, k), dV with
// (column length, d).  So the bits of a row of dQ depend only on that row's operands, those of a row of dK or dV only on its
// column's entries in CSR order and those rows' operands: not on sigma (the parent's or the companion's), any option, leading
// dimensions, alignment (16-byte loads only where every row of all four operands is 16-byte aligned; they feed the same chains)
// or the run.
//
// NON-FINITE values: a row whose forward output is NaN (Z = NaN) has r = NaN, so p and ds are NaN in all its entries: NaN in its
// dQ row and in the dK and dV rows of exactly the columns it stores.  A -Inf score has p = +0 * r = +0.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

// the kernel templates (csr5_attention_bwd_kern.h, shared with the biased entry point's translation unit
// csr5_attention_bwd_bias.hip)
#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher as well.
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
extern template AttBwdLaunch attention_bwd_launch<float, AttBwdArgs<float>>;
template AttBwdLaunch attention_bwd_launch<double, AttBwdArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
template AttBwdLaunch attention_bwd_launch<float, AttBwdArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
// heads == 1 is the single-head call: k_attention_bwd<VT, VEC, COL, false>
hipError_t launch_mha_bwd(const Geometry &g, const DeviceArrays &d, int value_type, const AttBwdCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_bwd_launch<double, AttBwdArgs<double>>(g, d, c, s);
    return attention_bwd_launch<float, AttBwdArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
