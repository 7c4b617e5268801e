// csr5_attention_bwd_edge.hip -- csr5hip_mha_edge_bias_backward: the gradients of csr5_attention_edge.hip's O for Q, K and V, and
// on request for the bias tensor B itself, in TWO launches, for gfx950 (wave64).  Per stored entry e = (i, j) and head h, every
// operation its own rounding:
//
//     s_e  = fma(qk_e, c, B[e * ldb + h]), the forward's score, the same bits (csr5_attention_edge.hip)
//     p_e, dp_e, D_i, ds_e = csr5_attention_bwd.hip's, with these scores
//     t_e  = ds_e * c                                   (one rounded multiplication)
//     dQ[i, c] = sum_e t_e K[j_e, c]      dK[j, c] = sum_e t_e Q[i_e, c]      dV[j, c] = sum_e p_e dO[i_e, c]
//     dB[e * lddb + h] = ds_e,h           (optional; the gradient of B: no reduction is needed)
//
// by csr5_attention_bwd.hip's accumulation rules, row classes, workspace and determinism contract: these are the same kernel
// templates (csr5_attention_bwd_kern.h) instantiated with an argument struct that carries B (AttBwdEdgeArgs); the plain and
// the biased instantiations are not touched by it.  THE ROW KERNEL reads B at the entry's CSR rank and writes dB exactly as the
// biased one writes dS (the extra sweep of a row beyond 2 048 entries included).  THE COLUMN KERNEL walks the transposed
// companion's pattern: the entry of rank j of companion line c sits at position q = t_row_ptr[c] + j of A^T's CSR order, and its
// rank in A's is e = map[q], map the companion's source map, which the C layer passes and nobody copies; so an entry has the
// same s, p and ds on both sides.  A lane of a short line loads e once and keeps it across the heads; the longer classes read
// the map word again per head (consecutive ranks, consecutive addresses) and then B[e * ldb + h], a scattered read.  THE
// HANDLE'S VALUES, THE PARENT'S AND THE COMPANION'S, ARE NOT READ.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_bwd_kern.h"

namespace csr5 {

// map: null for the row kernel, the companion's source map for the column kernel
template <typename VT, bool COL>
static hipError_t attention_bwd_edge_side(const Geometry &g, const DeviceArrays &d, AttBwdEdgeArgs<VT> A, const uint32_t *map,
                                          const int groups, const bool vec, hipStream_t s)
{
    if (g.m <= 0 || A.heads <= 0)
        return hipSuccess;
    attention_bwd_fill<VT>(A, g, d, groups);
    A.bias.map = map;
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    const dim3 grid(blocks, (unsigned)((A.heads + A.hper - 1) / A.hper)), block(AT_BLOCK);
    if (vec)
        hipLaunchKernelGGL((k_attention_bwd_edge<VT, true, COL>), grid, block, 0, s, A);
    else
        hipLaunchKernelGGL((k_attention_bwd_edge<VT, false, COL>), grid, block, 0, s, A);
    return hipGetLastError();
}

// g / d: the parent's pattern (the row kernel); gt / dt / map: the transposed companion's pattern and its source map (the column
// kernel, only when dK or dV is wanted: null otherwise).  The row kernel runs when dQ or dB is wanted or the column kernel needs
// the workspace.
template <typename VT>
static hipError_t attention_bwd_edge_typed(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt,
                                           const uint32_t *map, int heads, int groups, double scale, const void *B, int ldb,
                                           const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,
                                           const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv,
                                           void *work, void *dB, int lddb, hipStream_t s)
{
    AttBwdEdgeArgs<VT> A{};
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
    A.bias.B = (const VT *)B;
    A.bias.ldb = ldb;
    A.bias.c = (VT)scale;
    const bool vec = attention_bwd_vec<VT>(heads, k, dcols, Q, ldq, K, ldk, V, ldv, dO, lddo);
    const bool column = gt && dt && map && (dK || dV);
    hipError_t e = hipSuccess;
    if (dQ || dB || column) {
        AttBwdEdgeArgs<VT> R = A;
        R.dQ = k > 0 ? (VT *)dQ : nullptr;
        R.work = column ? (VT *)work : nullptr;
        R.dS = (VT *)dB;
        R.ldds = lddb;
        if (R.dQ || R.work || R.dS)
            e = attention_bwd_edge_side<VT, false>(g, d, R, nullptr, groups, vec, s);
    }
    if (e == hipSuccess && column) {
        AttBwdEdgeArgs<VT> C = A;
        C.dK = k > 0 ? (VT *)dK : nullptr;
        C.dV = dcols > 0 ? (VT *)dV : nullptr;
        C.work = (VT *)work;
        if (C.dK || C.dV)
            e = attention_bwd_edge_side<VT, true>(*gt, *dt, C, map, groups, vec, s);
    }
    return e;
}

// The product build compiles this file once per value type (-DCSR5_ATTENTION_BWD_ONLY_F64 / _F32), as csr5_attention_bwd.hip.
#define CSR5_BWD_EDGE_PARAMS                                                                                                              \
    const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, const uint32_t *map, int heads, int groups,     \
        double scale, const void *B, int ldb, const void *Q, int ldq, const void *K, int ldk, int k, const void *V, int ldv, int dcols,   \
        const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV, int lddv, void *work, void *dB, int lddb,             \
        hipStream_t s
#define CSR5_BWD_EDGE_ARGS                                                                                                                \
    g, d, gt, dt, map, heads, groups, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, dcols, dO, lddo, dQ, lddq, dK, lddk, dV, lddv, work, dB,  \
        lddb, s
#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_edge_bwd_f64(CSR5_BWD_EDGE_PARAMS) { return attention_bwd_edge_typed<double>(CSR5_BWD_EDGE_ARGS); }
#endif
#if !defined(CSR5_ATTENTION_BWD_ONLY_F64)
hipError_t launch_mha_edge_bwd_f32(CSR5_BWD_EDGE_PARAMS) { return attention_bwd_edge_typed<float>(CSR5_BWD_EDGE_ARGS); }
#endif

#if !defined(CSR5_ATTENTION_BWD_ONLY_F32)
hipError_t launch_mha_edge_bwd_f32(CSR5_BWD_EDGE_PARAMS);

hipError_t launch_mha_edge_bwd(const Geometry &g, const DeviceArrays &d, const Geometry *gt, const DeviceArrays *dt, const uint32_t *map,
                               int value_type, int heads, int groups, double scale, const void *B, int ldb, const void *Q, int ldq,
                               const void *K, int ldk, int k, const void *V, int ldv, int dcols, const void *dO, int lddo, void *dQ,
                               int lddq, void *dK, int lddk, void *dV, int lddv, void *work, void *dB, int lddb, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_mha_edge_bwd_f64(CSR5_BWD_EDGE_ARGS) : launch_mha_edge_bwd_f32(CSR5_BWD_EDGE_ARGS);
}
#endif
#undef CSR5_BWD_EDGE_PARAMS
#undef CSR5_BWD_EDGE_ARGS

} // namespace csr5
