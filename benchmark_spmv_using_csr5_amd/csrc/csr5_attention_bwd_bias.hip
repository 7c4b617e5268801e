// csr5_attention_bwd_bias.hip -- csr5hip_mha_biased_backward: the gradients of csr5_attention_bias.hip's O for Q, K and V, and on
// request for the biased score itself, in TWO launches, for gfx950 (wave64).  Per stored entry e = (i, j) and head h, every
// operation its own rounding:
//
//     s_e  = fma(qk_e, c, b_e), the forward's biased score, the same bits (csr5_attention_bias.hip)
//     p_e, dp_e, D_i, ds_e = csr5_attention_bwd.hip's, with these scores
//     t_e  = ds_e * c                                   (one rounded multiplication)
//     dQ[i, c] = sum_e t_e K[j_e, c]      dK[j, c] = sum_e t_e Q[i_e, c]      dV[j, c] = sum_e p_e dO[i_e, c]
//     dS[e * ldds + h] = ds_e,h           (optional; e the entry's CSR rank: the gradient for the biased score, before c and slope)
//
// by csr5_attention_bwd.hip's accumulation rules, row classes, workspace and determinism contract: these are the same kernel
// templates (csr5_attention_bwd_kern.h) instantiated with an argument struct that carries the bias (AttBwdBiasArgs); the plain
// instantiations are not touched by it.  THE ROW KERNEL reads the parent's values and writes dS (every (entry, head), a head
// group its own heads' elements, nothing beyond column heads - 1 of a row of dS); THE COLUMN KERNEL reads the transposed
// companion's values at the companion's storage position, so an entry has the same s, p and ds on both sides.  A row beyond
// 2 048 entries, whose ds exists only inside dQ's chunk refills, writes dS in one more sweep of the same recomputation.  The
// values are read, as in the forward, next to the column (kept across the heads by a lane of a short line, read again by every
// head otherwise), and never written.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

template <typename VT, bool COL>
static hipError_t attention_bwd_biased_side(const Geometry &g, const DeviceArrays &d, AttBwdBiasArgs<VT> A, const int groups,
                                            const bool vec, hipStream_t s)
{
    if (g.m <= 0 || A.heads <= 0)
        return hipSuccess;
    attention_bwd_fill<VT>(A, g, d, groups);
    A.bias.val = (const VT *)d.val;
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    const dim3 grid(blocks, (unsigned)((A.heads + A.hper - 1) / A.hper)), block(AT_BLOCK);
    if (vec)
        hipLaunchKernelGGL((k_attention_bwd_biased<VT, true, COL>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((k_attention_bwd_biased<VT, false, COL>), grid, block, 0, s, A);
    return hipGetLastError();
}

// g / d: the parent's pattern and values (the row kernel); gt / dt: the transposed companion's (the column kernel, only when dK or
// dV is wanted: null otherwise).  The row kernel runs when dQ or dS is wanted or the column kernel needs the workspace.
template <typename VT>
static hipError_t attention_bwd_biased_typed(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt,
                                             int heads, int groups, double scale, const void *slopes, const void *Q, int ldq,
                                             const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO, int lddo,
                                             void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, void *dS, int ldds,
                                             hipStream_t s)
{
    AttBwdBiasArgs<VT> A{};
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
    A.bias.slopes = (const VT *)slopes;
    A.bias.c = (VT)scale;
    const bool vec = attention_bwd_vec<VT>(heads, k, dcols, Q, ldq, K, ldk, V, ldv, dO, lddo);
    const bool column = gt && dt && (dK || dV);
    hipError_t e = hipSuccess;
    if (dQ || dS || column) {
        AttBwdBiasArgs<VT> R = A;
        R.dQ = k > 0 ? (VT *)dQ : nullptr;
        R.work = column ? (VT *)work : nullptr;
        R.dS = (VT *)dS;
        R.ldds = ldds;
        if (R.dQ || R.work || R.dS)
            e = attention_bwd_biased_side<VT, false>(g, d, R, groups, vec, s);
    }
    if (e == hipSuccess && column) {
        AttBwdBiasArgs<VT> C = A;
        C.dK = k > 0 ? (VT *)dK : nullptr;
        C.dV = dcols > 0 ? (VT *)dV : nullptr;
        C.work = (VT *)work;
        if (C.dK || C.dV)
            e = attention_bwd_biased_side<VT, true>(*gt, *dt, C, groups, vec, s);
    }
    return e;
}

// The product build compiles this file once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_attention_bwd.hip.
#define CSR5_BWD_BIASED_PARAMS                                                                                                            \
    const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int heads, int groups, double scale,            \
        const void *slopes, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO,     \
        int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, void *dS, int ldds, hipStream_t s
#define CSR5_BWD_BIASED_ARGS                                                                                                              \
    g, d, gt, dt, heads, groups, scale, slopes, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, work, dS, ldds, s
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_biased_bwd_f64(CSR5_BWD_BIASED_PARAMS) { return attention_bwd_biased_typed<double>(CSR5_BWD_BIASED_ARGS); }
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
hipError_t launch_mha_biased_bwd_f32(CSR5_BWD_BIASED_PARAMS) { return attention_bwd_biased_typed<float>(CSR5_BWD_BIASED_ARGS); }
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_biased_bwd_f32(CSR5_BWD_BIASED_PARAMS);

hipError_t launch_mha_biased_bwd(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, int value_type,
                                 int heads, int groups, double scale, const void *slopes, const void *Q, int ldq, const void *K, int ldk,
                                 int k, const void *V, int ldv, int dcols, const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk,
                                 void *dV, int lddv, void *work, void *dS, int ldds, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_mha_biased_bwd_f64(CSR5_BWD_BIASED_ARGS) : launch_mha_biased_bwd_f32(CSR5_BWD_BIASED_ARGS);
}
#endif
#undef CSR5_BWD_BIASED_PARAMS
#undef CSR5_BWD_BIASED_ARGS

} // namespace csr5
