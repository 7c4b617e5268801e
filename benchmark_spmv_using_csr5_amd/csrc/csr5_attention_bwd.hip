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

// g / d: the parent's pattern (the row kernel); gt / dt: the transposed companion's (the column kernel, only when dK or dV is
// wanted: null otherwise).  The row kernel runs when dQ is wanted or the column kernel needs the workspace.
template <typename VT>
static hipError_t attention_bwd_typed(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int heads,
                                      int groups, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,
                                      const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work,
                                      hipStream_t s)
{
    AttBwdArgs<VT> A{};
    A.k = k;
    A.d = dcols;
    A.heads = heads;
    A.ws = 4 * heads;
    A.Q = (const VT *)Q;
    A.K = (const VT *)K;
    A.V = (const VT *)V;
    A.dO = (const VT *)dO;
    A.ldq = ldq;
    A.ldk = ldk;
    A.ldv = ldv;
    A.lddo = lddo;
    A.lddq = lddq;
    A.lddk = lddk;
    A.lddv = lddv;
    const bool vec = attention_bwd_vec<VT>(heads, k, dcols, Q, ldq, K, ldk, V, ldv, dO, lddo);
    const bool column = gt && dt && (dK || dV);
    hipError_t e = hipSuccess;
    if (dQ || column) {
        AttBwdArgs<VT> R = A;
        R.dQ = k > 0 ? (VT *)dQ : nullptr;
        R.work = column ? (VT *)work : nullptr;
        if (R.dQ || R.work)
            e = attention_bwd_side<VT, false>(g, d, R, groups, vec, s);
    }
    if (e == hipSuccess && column) {
        AttBwdArgs<VT> C = A;
        C.dK = k > 0 ? (VT *)dK : nullptr;
        C.dV = dcols > 0 ? (VT *)dV : nullptr;
        C.work = (VT *)work;
        if (C.dK || C.dV)
            e = attention_bwd_side<VT, true>(*gt, *dt, C, groups, vec, s);
    }
    return e;
}

// The product build compiles this file once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_attention.hip.
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_bwd_f64(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int heads, int groups,
                              const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO,
                              int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, hipStream_t s)
{
    return attention_bwd_typed<double>(g, d, gt, dt, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq, dK, lddk, dV,
                                       lddv, work, s);
}
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
hipError_t launch_mha_bwd_f32(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int heads, int groups,
                              const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO,
                              int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, hipStream_t s)
{
    return attention_bwd_typed<float>(g, d, gt, dt, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq, dK, lddk, dV,
                                      lddv, work, s);
}
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_bwd_f32(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int heads, int groups,
                              const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO,
                              int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, hipStream_t s);

hipError_t launch_mha_bwd(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int value_type, int heads,
                          int groups, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,
                          const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_mha_bwd_f64(g, d, gt, dt, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq,
                                                          dK, lddk, dV, lddv, work, s)
                                     : launch_mha_bwd_f32(g, d, gt, dt, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq,
                                                          dK, lddk, dV, lddv, work, s);
}

hipError_t launch_attention_bwd(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int value_type,
                                const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO,
                                int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, hipStream_t s)
{
    return launch_mha_bwd(g, d, gt, dt, value_type, 1, 0, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, work,
                          s);
}
#endif

} // namespace csr5
