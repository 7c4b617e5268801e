// csr5_attention_bwd_kern.h -- the kernel templates of the attention backward on the pattern and the launcher of one side; the
// contract is written out at the head of csr5_attention_bwd.hip.  Two translation units instantiate them: csr5_attention_bwd.hip
// the plain entry points (AttBwdArgs), csr5_attention_bwd_bias.hip the biased one (csr5hip_mha_biased_backward; AttBwdBiasArgs),
// csr5_attention_bwd_edge.hip the edge-biased one (csr5hip_mha_edge_bias_backward; AttBwdEdgeArgs: ARGS::EDGE).
// csr5_attention_bwd_lowp.hip instantiates them a fourth time with operands and outputs STORED in bf16 or fp16 and float arithmetic
// (csr5hip_mha_lowp_backward; AttBwdLowpArgs, k_attention_bwd_lowp): ARGS::ST is the type behind the operand and output pointers, VT
// the type of everything computed, of the workspace, the LDS stage and the reductions.  Where ST == VT the casts between them and
// att_stored are no operation, and the kernels of the other units are, instruction for instruction, what they were without them
// (scripts/compare_attention_asm.py).
// THE BIAS IS A COMPILE-TIME PROPERTY OF THE ARGUMENT STRUCT (ARGS::BIASED), as in csr5_attention_kern.h: the plain instantiations
// carry no argument, no branch and no load for it.  csr5_attention_bwd_drop_lowp.hip: the 16-bit backward under the dropout mask
// (csr5hip_dropout_mha_lowp_backward; AttBwdLowpDropArgs, k_attention_bwd_lowp_drop).  Include it after `#pragma clang fp contract(off)`; gfx950 (wave64) only.
#pragma once

#include "csr5_attention_dev.h"

namespace csr5 {

template <typename VT>
struct AttBwdArgs {
    static constexpr bool BIASED = false;
    static constexpr bool EDGE = false; // (with BIASED: the bias is AttEdgeBias, read at the entry's rank in the parent's CSR order)
    static constexpr bool GAT = false;  // (with EDGE: the additive score of AttBwdGatArgs in place of the dot product)
    static constexpr bool DROP = false; // (with EDGE: the dropout mask of AttBwdDropArgs / AttBwdDropGatArgs)
    using ST = VT;                      // the type behind the operand and output pointers (AttBwdLowpArgs: another one than VT)
    int lines, k, d;     // lines: rows of the pattern walked (m in the row kernel, n in the column kernel)
    int T, sigma, tiles; // tile_elems, sigma, p - 1 of that pattern
    unsigned recip;
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const VT *Q, *K, *V, *dO;
    VT *dQ, *dK, *dV; // row kernel: dQ or null; column kernel: dK, dV, one of them may be null
    VT *work;         // [4 m heads]: M, r, D and one unused value per (row of A, head), a row's heads adjacent; the row kernel writes
                      // (null: not wanted), the column kernel reads
    int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
    int heads, hper;  // heads of the packed operands; heads of one workgroup (blockIdx.y owns heads y hper .. y hper + hper - 1)
    int ws;           // 4 heads: the workspace values of one row
};

// csr5hip_mha_biased_backward: s = fma(qk, c, slope_h * a_e) (att_bias_score), the accumulations take t_e = ds_e * c, and the
// row kernel writes ds_e to dS[e * ldds + h], e the entry's CSR rank, when dS is wanted (null: not wanted; the column kernel's
// is always null).  bias.val: the values of the pattern walked -- the parent's in the row kernel, the companion's in the column kernel.
template <typename VT>
struct AttBwdBiasArgs : AttBwdArgs<VT> {
    static constexpr bool BIASED = true;
    AttBias<VT> bias;
    VT *dS;
    int ldds;
};

// csr5hip_mha_edge_bias_backward: s = fma(qk, c, B[e * ldb + h]), e the entry's rank in the PARENT's CSR order: the position
// walked in the row kernel (bias.map null), map[position walked] in the column kernel (bias.map the companion's source map), so
// that an entry has the same s, p and ds on both sides.  dS / ldds are the call's dB / lddb: ds_e,h IS the gradient of B[e, h],
// written by the row kernel by the biased rule.  Nothing of the handle's values is read.
template <typename VT>
struct AttBwdEdgeArgs : AttBwdArgs<VT> {
    static constexpr bool BIASED = true;
    static constexpr bool EDGE = true;
    AttEdgeBias<VT> bias;
    VT *dS;
    int ldds;
};

// csr5hip_gat_backward (csr5_attention_bwd_gat.hip): the edge call with s = fma(z, c, B[e, h]), z the additive score's chain
// (att_gat_z).  p, dp, D, ds, t, dV and dS / dB are the edge call's with these scores.  u_c = Q[i, c] + K[j, c] and l_c are recomputed
// where they are needed, the forward's bits on both sides; the accumulations take the operand w_c = a_c g_c, g_c = u_c > 0 ? 1 : ns,
// in K's / Q's place (gat_short_acc, gat_wave_acc, gat_hub_acc), and the row kernel accumulates t_e l_ec next to t_e w_ec into
// dAr[i * lddar + h k + c], the row's share of a's gradient (null: not wanted).
template <typename VT>
struct AttBwdGatArgs : AttBwdEdgeArgs<VT> {
    static constexpr bool GAT = true;
    AttGat<VT> gat;
    VT *dAr;
    int lddar;
};

// csr5hip_mha_lowp_backward (csr5_attention_bwd_lowp.hip): AttBwdEdgeArgs<float>'s call with Q, K, V, B and dO STORED in ST (bf16 or
// fp16) and dQ, dK, dV and dB written in it.  The arithmetic, the LDS stage, the reductions and the workspace are float: the templates
// below widen an operand where they load it and round an output once where they store it (att_stored), and are otherwise the float
// instantiation's, statement for statement.  A struct of its own: the existing ones keep their layouts, and their kernels their code.
template <typename ST_>
struct AttBwdLowpArgs {
    static constexpr bool BIASED = true;
    static constexpr bool EDGE = true;
    static constexpr bool GAT = false;
    static constexpr bool DROP = false;
    using ST = ST_;
    int lines, k, d;
    int T, sigma, tiles;
    unsigned recip;
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const ST *Q, *K, *V, *dO;
    ST *dQ, *dK, *dV;
    float *work; // unrounded: the column kernel reads back the row kernel's M, 1 / Z and D
    int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
    int heads, hper;
    int ws;
    AttEdgeBiasLowpMap<ST> bias;
    ST *dS;
    int ldds;
};

// csr5hip_dropout_mha_backward (csr5_attention_bwd_drop.hip) and csr5hip_dropout_gat_backward (csr5_attention_bwd_drop_gat.hip): the
// edge call's and the additive one's gradients under the forward's dropout mask (csr5_attention_dev.h AttDrop), recomputed per entry
// and head from the entry's rank in the PARENT's CSR order -- the position walked in the row kernel, map[position] in the column
// kernel.  g_e = keep ? cd : +0; dp_e = g_e * (dO_i . V_j chain), one multiplication, on both sides; p, D and ds follow from it as
// they always do; dV's coefficient is p_e * g_e, one multiplication, in p_e's place.  The workspace keeps its meaning.
template <typename VT>
struct AttBwdDropArgs : AttBwdEdgeArgs<VT> {
    static constexpr bool DROP = true;
    AttDrop<VT> drop;
};
template <typename VT>
struct AttBwdDropGatArgs : AttBwdGatArgs<VT> {
    static constexpr bool DROP = true;
    AttDrop<VT> drop;
};

// csr5hip_dropout_mha_lowp_backward (csr5_attention_bwd_drop_lowp.hip): AttBwdDropArgs<float>'s call on operands and outputs stored in
// ST -- the 16-bit backward under the forward's mask, derived as AttBwdDropArgs is from the edge struct.  g, cd and the workspace are
// float; the column kernel takes the entry's rank from the lowp bias struct's map
template <typename ST_>
struct AttBwdLowpDropArgs : AttBwdLowpArgs<ST_> {
    static constexpr bool DROP = true;
    AttDrop<float> drop;
};

// the arguments of head h alone: every operand moved to that head's slice, the workspace to that head's values of row 0 (biased:
// the slopes and dS to that head's element, so that head 0 of the result is head h)
template <typename ARGS>
__device__ __forceinline__ ARGS bwd_head(const ARGS &A, const int h)
{
    ARGS H = A;
    const size_t ok = (size_t)h * A.k, od = (size_t)h * A.d;
    H.Q += ok;
    H.K += ok;
    H.V += od;
    H.dO += od;
    if (H.dQ)
        H.dQ += ok;
    if (H.dK)
        H.dK += ok;
    if (H.dV)
        H.dV += od;
    if (H.work)
        H.work += 4 * (size_t)h;
    if constexpr (ARGS::GAT) {
        if (H.gat.a)
            H.gat.a += ok;
        if (H.dAr)
            H.dAr += ok;
    }
    if constexpr (ARGS::DROP)
        H.drop.key.head0 += (uint32_t)h;
    if constexpr (ARGS::EDGE) {
        if (H.bias.B)
            H.bias.B += h;
        if (H.dS)
            H.dS += h;
    } else if constexpr (ARGS::BIASED) {
        if (H.bias.slopes)
            H.bias.slopes += h;
        if (H.dS)
            H.dS += h;
    }
    return H;
}

// biased: the value of the entry of rank j of a line, from the value array at the storage position its column is read from --
// by every head again: unlike the columns the values are not staged; plain: nothing is read.  Edge-biased: the bias of head 0 of
// A of that entry, from B at the entry's rank in the parent's CSR order (the column kernel reads the map word first)
template <typename VT, typename ARGS>
__device__ __forceinline__ VT bwd_value(const ARGS &A, const int t0, const int rem0, const int j)
{
    if constexpr (ARGS::EDGE)
        return att_edge_value(A.bias, att_edge_rank(A.bias, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j), 0);
    else if constexpr (ARGS::BIASED)
        return A.bias.val[att_storage(A, t0, rem0, j)];
    else
        return (VT)0;
}

// dropout: g_e of head 0 of A of the entry of rank j of the line, keep ? cd : +0; otherwise nothing is computed
template <typename VT, typename ARGS>
__device__ __forceinline__ VT bwd_drop_g(const ARGS &A, const int t0, const int rem0, const int j)
{
    if constexpr (ARGS::DROP)
        return att_drop_factor(A.drop, att_edge_rank(A.bias, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j), 0);
    else
        return (VT)1;
}

// the coefficient of dQ and dK: ds, biased t = ds * c (one rounded multiplication)
template <typename VT, typename ARGS>
__device__ __forceinline__ VT bwd_coef(const ARGS &A, const VT ds)
{
    if constexpr (ARGS::BIASED)
        return ds * A.bias.c;
    else
        return ds;
}

// the row kernel's dS: ds of the entry of rank j of the line that starts at CSR rank t0 T + rem0, head 0 of A
template <typename VT, typename ARGS>
__device__ __forceinline__ void bwd_store_ds(const ARGS &A, const int t0, const int rem0, const int j, const VT ds)
{
    if constexpr (ARGS::BIASED)
        if (A.dS)
            A.dS[((size_t)t0 * A.T + (size_t)rem0 + (size_t)j) * A.ldds] = att_stored<typename ARGS::ST>(ds);
}

// whether the chains of an instantiation take a 32-byte block in two halves (att_score's HALVES): the dropped bf16 kernels only --
// false, and att_score's code untouched, for every other argument struct.  (fp16 has no scratch without it and is 4 to 8 % faster
// that way: DESIGN.md section 31)
template <typename VT, typename ARGS>
constexpr bool bwd_halves = ARGS::DROP && __is_same(typename ARGS::ST, __bf16);

// the score of the entry (i, j) alone; av: its value (read only when biased)
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ VT bwd_score(const ARGS &A, const size_t i, const size_t j, const VT av)
{
    if constexpr (ARGS::GAT) {
        return att_bias_score(A.bias, 0, att_gat_z<VT>(A.Q + i * A.ldq, A.K + j * A.ldk, A.gat.a, A.gat.ns, A.k), av);
    } else {
        const VT s = att_score<VT, VEC, bwd_halves<VT, ARGS>>(A.Q + i * A.ldq, A.K + j * A.ldk, A.k);
        if constexpr (ARGS::BIASED)
            return att_bias_score(A.bias, 0, s, av);
        else
            return s;
    }
}

// s_e and dp_e of the entry (i, j); av: its value (read only when biased); g: its dropout factor (used only with ARGS::DROP)
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void bwd_entry(const ARGS &A, const size_t i, const size_t j, const VT av, const VT g, VT &s, VT &dp)
{
    s = bwd_score<VT, VEC>(A, i, j, av);
    dp = att_score<VT, VEC, bwd_halves<VT, ARGS>>(A.dO + i * A.lddo, A.V + j * A.ldv, A.d);
    if constexpr (ARGS::DROP)
        dp = g * dp;
}

// p_e and ds_e (biased: t_e = ds_e * c, dK's coefficient) of the entry (i, j) from the workspace values of row i: the column
// kernel's entry.  With ARGS::DROP p leaves as dV's coefficient, p_e * g
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void bwd_entry_col(const ARGS &A, const size_t i, const size_t j, const VT av, const VT g, VT &p, VT &ds)
{
    const VT *wk = A.work + (size_t)A.ws * i;
    const VT M = wk[0], r = wk[1], D = wk[2];
    VT s, dp;
    bwd_entry<VT, VEC>(A, i, j, av, g, s, dp);
    p = exp_vt(s - M) * r;
    ds = bwd_coef(A, p * (dp - D));
    if constexpr (ARGS::DROP)
        p = p * g;
}

// ---- accumulation, L <= 16: ONE chain per output column over the entries in ascending order.  coef / idx: lane sub * 16 + e
// holds the coefficient and the operand row of entry e; out: the output row (used where rowok)
template <typename VT, typename ST>
__device__ __forceinline__ void bwd_short_acc(const bool rowok, const int rl, const int sub, const int pos, const VT coef, const int idx,
                                              const ST *__restrict__ X, const int ldx, const int width, ST *out)
{
    constexpr int G = AT_G;
    for (int cb = 0; cb < width; cb += G) { // (uniform)
        const int c = cb + pos;
        VT acc = (VT)0;
        for (int e = 0; e < G; e++) {
            if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                break;
            const VT we = __shfl(coef, sub * G + e, OMEGA);
            const int je = __shfl(idx, sub * G + e, OMEGA);
            if (rowok && e < rl && c < width)
                acc = fma_vt(we, (VT)X[(size_t)(uint32_t)je * ldx + c], acc);
        }
        if (rowok && c < width)
            out[c] = att_stored<ST>(acc);
    }
}

// ---- accumulation, 17 <= L <= 512: the forward's wavefront rule; coef / idx: the wavefront's staged entries in LDS
template <typename VT, typename ST>
__device__ __forceinline__ void bwd_wave_acc(const VT *coef, const int *idx, const int rl, const ST *__restrict__ X, const int ldx,
                                             const int width, ST *out)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int cb = 0; cb < width; cb += OMEGA) {
        const int wb = width - cb < OMEGA ? width - cb : OMEGA;
        const int C = att_pow2(wb), S = OMEGA / C;
        const int slot = lane / C, cc = lane & (C - 1);
        VT acc = (VT)0;
        if (cc < wb) {
            const ST *x = X + cb + cc;
#pragma unroll 4
            for (int e = slot; e < rl; e += S)
                acc = fma_vt(coef[e], (VT)x[(size_t)(uint32_t)idx[e] * ldx], acc);
        }
        for (int off = C; off < OMEGA; off <<= 1) // (uniform; adjacent slots first)
            acc += __shfl_xor(acc, off, OMEGA);
        if (slot == 0 && cc < wb)
            out[cb + cc] = att_stored<ST>(acc);
    }
}

// ---- accumulation, L > 512: the forward's workgroup rule.  staged: coef / idx hold all rl entries (filled by the caller; the
// barrier below publishes them); otherwise fill(base, n) writes entries base .. base + n - 1 to coef / idx [0, n) chunk by chunk,
// again for every 256 output columns.  Ends with a barrier: the stage is free.
template <typename VT, typename FILL, typename ST>
__device__ __forceinline__ void bwd_hub_acc(const int rl, const bool staged, FILL fill, const VT *coef, const int *idx,
                                            const ST *__restrict__ X, const int ldx, const int width, ST *out, VT *red)
{
    const int tid = (int)threadIdx.x;
    for (int cg = 0; cg < width; cg += OMEGA * AT_HUB_BLOCKS) {
        VT acc[AT_HUB_BLOCKS];
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++)
            acc[b] = (VT)0;
        for (int base = 0; base < rl; base += AT_STAGE) {
            const int n = rl - base < AT_STAGE ? rl - base : AT_STAGE;
            if (!staged) {
                __syncthreads(); // (the stage is free: the previous chunk has been read)
                fill(base, n);
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < AT_HUB_BLOCKS; b++) {
                const int cb = cg + b * OMEGA;
                if (cb < width) {
                    const int wb = width - cb < OMEGA ? width - cb : OMEGA;
                    const int C = att_pow2(wb), S = AT_BLOCK / C; // (AT_STAGE is a multiple of S: a chunk keeps j mod S)
                    const int slot = tid / C, cc = tid & (C - 1);
                    if (cc < wb) {
                        const ST *x = X + cb + cc;
                        VT o = acc[b];
#pragma unroll 4
                        for (int e = slot; e < n; e += S)
                            o = fma_vt(coef[e], (VT)x[(size_t)(uint32_t)idx[e] * ldx], o);
                        acc[b] = o;
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            const int cb = cg + b * OMEGA;
            if (cb < width) { // (uniform)
                const int wb = width - cb < OMEGA ? width - cb : OMEGA;
                const int C = att_pow2(wb);
                VT o = acc[b];
                for (int off = C; off < OMEGA; off <<= 1) // adjacent slots of the wavefront first ...
                    o += __shfl_xor(o, off, OMEGA);
                red[tid] = o;
                __syncthreads();
                if (tid < wb) // ... then (w0 + w1) + (w2 + w3); lane c < C of every wavefront holds column c
                    out[cb + tid] = att_stored<ST>((red[tid] + red[OMEGA + tid]) + (red[2 * OMEGA + tid] + red[3 * OMEGA + tid]));
                __syncthreads(); // (red is free for the next block)
            }
        }
    }
    __syncthreads();
}

// ---- the additive score's accumulations (ARGS::GAT): bwd_short_acc, bwd_wave_acc and bwd_hub_acc with the operand of entry e and
// column c computed instead of loaded: u = Q's element + K's (X[idx[e]] holds one of them, self -- the line's own row of Q in the
// row kernel, of K in the column kernel -- the other; Q's first, as the forward adds them), g = u > 0 ? 1 : ns, w = a_c * g (one
// rounding; a null: w = g), acc = fma(coef_e, w, acc).  The orders are those routines', so dQ and dK keep mha_backward's accumulation
// rules.  SECOND (the row kernel): a second chain acc2 = fma(coef_e, l, acc2), l = LeakyReLU(u), in the same order, written to out2.
// out / out2: null when not wanted (at least one is).
template <typename VT, bool COL>
__device__ __forceinline__ VT gat_u(const VT x, const VT self)
{
    return COL ? x + self : self + x;
}

template <typename VT, bool COL, bool SECOND>
__device__ __forceinline__ void gat_short_acc(const bool rowok, const int rl, const int sub, const int pos, const VT coef, const int idx,
                                              const VT *__restrict__ X, const int ldx, const VT *__restrict__ self,
                                              const VT *__restrict__ av, const VT ns, const int width, VT *out, VT *out2)
{
    constexpr int G = AT_G;
    for (int cb = 0; cb < width; cb += G) { // (uniform)
        const int c = cb + pos;
        VT acc = (VT)0, acc2 = (VT)0, y = (VT)0, ac = (VT)1;
        if (rowok && c < width) {
            y = self[c];
            if (av)
                ac = av[c];
        }
        for (int e = 0; e < G; e++) {
            if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                break;
            const VT we = __shfl(coef, sub * G + e, OMEGA);
            const int je = __shfl(idx, sub * G + e, OMEGA);
            if (rowok && e < rl && c < width) {
                const VT u = gat_u<VT, COL>(X[(size_t)(uint32_t)je * ldx + c], y);
                const VT g = u > (VT)0 ? (VT)1 : ns;
                acc = fma_vt(we, av ? ac * g : g, acc);
                if constexpr (SECOND)
                    acc2 = fma_vt(we, att_gat_leaky(u, ns), acc2);
            }
        }
        if (rowok && c < width) {
            if (out)
                out[c] = acc;
            if constexpr (SECOND)
                if (out2)
                    out2[c] = acc2;
        }
    }
}

template <typename VT, bool COL, bool SECOND>
__device__ __forceinline__ void gat_wave_acc(const VT *coef, const int *idx, const int rl, const VT *__restrict__ X, const int ldx,
                                             const VT *__restrict__ self, const VT *__restrict__ av, const VT ns, const int width,
                                             VT *out, VT *out2)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int cb = 0; cb < width; cb += OMEGA) {
        const int wb = width - cb < OMEGA ? width - cb : OMEGA;
        const int C = att_pow2(wb), S = OMEGA / C;
        const int slot = lane / C, cc = lane & (C - 1);
        VT acc = (VT)0, acc2 = (VT)0;
        if (cc < wb) {
            const VT *x = X + cb + cc;
            const VT y = self[cb + cc];
            const VT ac = av ? av[cb + cc] : (VT)1;
#pragma unroll 4
            for (int e = slot; e < rl; e += S) {
                const VT u = gat_u<VT, COL>(x[(size_t)(uint32_t)idx[e] * ldx], y);
                const VT g = u > (VT)0 ? (VT)1 : ns;
                acc = fma_vt(coef[e], av ? ac * g : g, acc);
                if constexpr (SECOND)
                    acc2 = fma_vt(coef[e], att_gat_leaky(u, ns), acc2);
            }
        }
        for (int off = C; off < OMEGA; off <<= 1) { // (uniform; adjacent slots first)
            acc += __shfl_xor(acc, off, OMEGA);
            if constexpr (SECOND)
                acc2 += __shfl_xor(acc2, off, OMEGA);
        }
        if (slot == 0 && cc < wb) {
            if (out)
                out[cb + cc] = acc;
            if constexpr (SECOND)
                if (out2)
                    out2[cb + cc] = acc2;
        }
    }
}

template <typename VT, bool COL, bool SECOND, typename FILL>
__device__ __forceinline__ void gat_hub_acc(const int rl, const bool staged, FILL fill, const VT *coef, const int *idx,
                                            const VT *__restrict__ X, const int ldx, const VT *__restrict__ self,
                                            const VT *__restrict__ av, const VT ns, const int width, VT *out, VT *out2, VT *red)
{
    const int tid = (int)threadIdx.x;
    for (int cg = 0; cg < width; cg += OMEGA * AT_HUB_BLOCKS) {
        VT acc[AT_HUB_BLOCKS], acc2[AT_HUB_BLOCKS];
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            acc[b] = (VT)0;
            acc2[b] = (VT)0;
        }
        for (int base = 0; base < rl; base += AT_STAGE) {
            const int n = rl - base < AT_STAGE ? rl - base : AT_STAGE;
            if (!staged) {
                __syncthreads(); // (the stage is free: the previous chunk has been read)
                fill(base, n);
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < AT_HUB_BLOCKS; b++) {
                const int cb = cg + b * OMEGA;
                if (cb < width) {
                    const int wb = width - cb < OMEGA ? width - cb : OMEGA;
                    const int C = att_pow2(wb), S = AT_BLOCK / C; // (AT_STAGE is a multiple of S: a chunk keeps j mod S)
                    const int slot = tid / C, cc = tid & (C - 1);
                    if (cc < wb) {
                        const VT *x = X + cb + cc;
                        const VT y = self[cb + cc];
                        const VT ac = av ? av[cb + cc] : (VT)1;
                        VT o = acc[b], o2 = acc2[b];
#pragma unroll 4
                        for (int e = slot; e < n; e += S) {
                            const VT u = gat_u<VT, COL>(x[(size_t)(uint32_t)idx[e] * ldx], y);
                            const VT g = u > (VT)0 ? (VT)1 : ns;
                            o = fma_vt(coef[e], av ? ac * g : g, o);
                            if constexpr (SECOND)
                                o2 = fma_vt(coef[e], att_gat_leaky(u, ns), o2);
                        }
                        acc[b] = o;
                        acc2[b] = o2;
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            const int cb = cg + b * OMEGA;
            if (cb < width) { // (uniform)
                const int wb = width - cb < OMEGA ? width - cb : OMEGA;
                const int C = att_pow2(wb);
                for (int second = 0; second < (SECOND ? 2 : 1); second++) { // (uniform)
                    VT o = second ? acc2[b] : acc[b];
                    VT *dst = second ? out2 : out;
                    for (int off = C; off < OMEGA; off <<= 1) // adjacent slots of the wavefront first ...
                        o += __shfl_xor(o, off, OMEGA);
                    red[tid] = o;
                    __syncthreads();
                    if (tid < wb && dst) // ... then (w0 + w1) + (w2 + w3); lane c < C of every wavefront holds column c
                        dst[cb + tid] = (red[tid] + red[OMEGA + tid]) + (red[2 * OMEGA + tid] + red[3 * OMEGA + tid]);
                    __syncthreads(); // (red is free for the next block)
                }
            }
        }
    }
    __syncthreads();
}

// ---- lines of at most 16 entries (empty ones included): 16 lanes per line, 4 lines of the wavefront per pass ---------------
template <typename VT, bool VEC, bool COL, typename ARGS>
__device__ __forceinline__ void bwd_short(const ARGS &A0, const long long row0, const int len, const int t0, const int rem0,
                                          const int h0, const int h1)
{
    constexpr int G = AT_G, ROWS = OMEGA / G;
    const int lane = threadIdx.x & (OMEGA - 1);
    const int sub = lane / G, pos = lane % G;
    const unsigned long long cls = __ballot(len >= 0 && len <= G); // (len = -1: no such line)
    if (!cls)
        return;
    for (int pass = 0; pass < G; pass++) {
        const unsigned long long here = (cls >> (pass * ROWS)) & ((1ull << ROWS) - 1);
        if (!here) // (wave-uniform)
            continue;
        const int src = pass * ROWS + sub;
        const int rl = __shfl(len, src, OMEGA);
        const int rt0 = __shfl(t0, src, OMEGA);
        const int rrem = __shfl(rem0, src, OMEGA);
        const bool rowok = (cls >> src) & 1;
        const bool act = rowok && pos < rl;
        const size_t r = (size_t)(row0 + src);
        int other = 0; // the lane's column (and, biased, its value; edge-biased, its rank): loaded once, kept across the heads
        VT av = (VT)0;
        size_t er = 0;
        if (act)
            other = A0.col[att_storage(A0, rt0, rrem, pos)];
        if constexpr (ARGS::EDGE) {
            if (act)
                er = att_edge_rank(A0.bias, (size_t)rt0 * A0.T + (size_t)rrem + (size_t)pos);
        } else if constexpr (ARGS::BIASED) {
            if (act)
                av = bwd_value<VT>(A0, rt0, rrem, pos);
        }
        for (int h = h0; h < h1; h++) { // (uniform)
            const ARGS A = bwd_head(A0, h);
            if constexpr (ARGS::EDGE)
                if (act)
                    av = att_edge_value(A.bias, er, 0);
            VT g = (VT)1;
            if constexpr (ARGS::DROP)
                if (act)
                    g = att_drop_factor(A.drop, er, 0);
            if constexpr (COL) {
                VT p = (VT)0, ds = (VT)0;
                if (act)
                    bwd_entry_col<VT, VEC>(A, (size_t)(uint32_t)other, r, av, g, p, ds);
                if (A.dV)
                    bwd_short_acc<VT>(rowok, rl, sub, pos, p, other, A.dO, A.lddo, A.d, A.dV + r * A.lddv);
                if constexpr (ARGS::GAT) {
                    if (A.dK)
                        gat_short_acc<VT, true, false>(rowok, rl, sub, pos, ds, other, A.Q, A.ldq, A.K + r * A.ldk, A.gat.a, A.gat.ns,
                                                       A.k, A.dK + r * A.lddk, nullptr);
                } else if (A.dK)
                    bwd_short_acc<VT>(rowok, rl, sub, pos, ds, other, A.Q, A.ldq, A.k, A.dK + r * A.lddk);
            } else {
                VT s = neg_inf<VT>(), dp = (VT)0;
                if (act)
                    bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)other, av, g, s, dp);
                const VT mx = group_max<G>(s);
                const VT w = act ? exp_vt(s - mx) : (VT)0;
                const VT rinv = (VT)1 / group_sum<G>(w);
                const VT p = act ? w * rinv : (VT)0;
                const VT pg = p * dp;
                const VT D = group_sum<G>(act ? pg : (VT)0);
                const VT ds = act ? p * (dp - D) : (VT)0;
                if (A.work && rowok && pos == 0) {
                    VT *wk = A.work + (size_t)A.ws * r;
                    wk[0] = mx;
                    wk[1] = rinv;
                    wk[2] = D;
                }
                if (act)
                    bwd_store_ds(A, rt0, rrem, pos, ds);
                if constexpr (ARGS::GAT) {
                    if (A.dQ || A.dAr)
                        gat_short_acc<VT, false, true>(rowok, rl, sub, pos, bwd_coef(A, ds), other, A.K, A.ldk, A.Q + r * A.ldq,
                                                       A.gat.a, A.gat.ns, A.k, A.dQ ? A.dQ + r * A.lddq : nullptr,
                                                       A.dAr ? A.dAr + r * A.lddar : nullptr);
                } else if (A.dQ)
                    bwd_short_acc<VT>(rowok, rl, sub, pos, bwd_coef(A, ds), other, A.K, A.ldk, A.k, A.dQ + r * A.lddq);
            }
        }
    }
}

// ---- a line of 17 .. 512 entries: one wavefront; a / b / cl: the wavefront's 512 staged values, values and indices ---------
// One head: A holds that head's slices; first: the head that stages cl, which the later heads read back (a lane its own entries).
template <typename VT, bool VEC, bool COL, typename ARGS>
__device__ __forceinline__ void bwd_wave_head(const ARGS &A, const bool first, const size_t r, const int rl, const int t0,
                                              const int rem0, VT *a, VT *b, int *cl)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    if constexpr (COL) {
        for (int j = lane; j < rl; j += OMEGA) {
            const int i = first ? A.col[att_storage(A, t0, rem0, j)] : cl[j];
            const VT av = bwd_value<VT>(A, t0, rem0, j);
            VT p, ds;
            bwd_entry_col<VT, VEC>(A, (size_t)(uint32_t)i, r, av, bwd_drop_g<VT>(A, t0, rem0, j), p, ds);
            a[j] = p;
            b[j] = ds;
            cl[j] = i;
        }
        att_wave_sync();
        if (A.dV)
            bwd_wave_acc<VT>(a, cl, rl, A.dO, A.lddo, A.d, A.dV + r * A.lddv);
        if constexpr (ARGS::GAT) {
            if (A.dK)
                gat_wave_acc<VT, true, false>(b, cl, rl, A.Q, A.ldq, A.K + r * A.ldk, A.gat.a, A.gat.ns, A.k, A.dK + r * A.lddk,
                                              nullptr);
        } else if (A.dK)
            bwd_wave_acc<VT>(b, cl, rl, A.Q, A.ldq, A.k, A.dK + r * A.lddk);
    } else {
        VT mx = neg_inf<VT>();
        for (int j = lane; j < rl; j += OMEGA) {
            const int cj = first ? A.col[att_storage(A, t0, rem0, j)] : cl[j];
            const VT av = bwd_value<VT>(A, t0, rem0, j);
            VT s, dp;
            bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)cj, av, bwd_drop_g<VT>(A, t0, rem0, j), s, dp);
            a[j] = s;
            b[j] = dp;
            cl[j] = cj;
            mx = max_vt(mx, s);
        }
        mx = wave_max(mx);
        VT z = (VT)0;
        for (int j = lane; j < rl; j += OMEGA) { // (a lane reads back what it stored itself, here and below)
            const VT w = exp_vt(a[j] - mx);
            a[j] = w;
            z += w;
        }
        const VT rinv = (VT)1 / wave_sum(z);
        VT dsum = (VT)0;
        for (int j = lane; j < rl; j += OMEGA) {
            const VT p = a[j] * rinv;
            const VT pg = p * b[j];
            a[j] = p;
            dsum += pg;
        }
        const VT D = wave_sum(dsum);
        for (int j = lane; j < rl; j += OMEGA) {
            const VT ds = a[j] * (b[j] - D);
            bwd_store_ds(A, t0, rem0, j, ds);
            a[j] = bwd_coef(A, ds);
        }
        if (A.work && lane == 0) {
            VT *wk = A.work + (size_t)A.ws * r;
            wk[0] = mx;
            wk[1] = rinv;
            wk[2] = D;
        }
        att_wave_sync();
        if constexpr (ARGS::GAT) {
            if (A.dQ || A.dAr)
                gat_wave_acc<VT, false, true>(a, cl, rl, A.K, A.ldk, A.Q + r * A.ldq, A.gat.a, A.gat.ns, A.k,
                                              A.dQ ? A.dQ + r * A.lddq : nullptr, A.dAr ? A.dAr + r * A.lddar : nullptr);
        } else if (A.dQ)
            bwd_wave_acc<VT>(a, cl, rl, A.K, A.ldk, A.k, A.dQ + r * A.lddq);
    }
    att_wave_sync(); // (the next head's and the next line's entries stay behind these reads)
}

template <typename VT, bool VEC, bool COL, typename ARGS>
__device__ __forceinline__ void bwd_wave_line(const ARGS &A, const size_t r, const int rl, const int t0, const int rem0, VT *a,
                                              VT *b, int *cl, const int h0, const int h1)
{
    for (int h = h0; h < h1; h++) // (uniform)
        bwd_wave_head<VT, VEC, COL>(bwd_head(A, h), h == h0, r, rl, t0, rem0, a, b, cl);
}

// ---- a line beyond 512 entries: the workgroup; a / b / cl: the AT_STAGE staged entries, red: AT_BLOCK values, red4: AT_WAVES
// One head: A holds that head's slices; first: the head that stages cl of a line of at most AT_STAGE entries, which the later
// heads read back (beyond AT_STAGE entries the stage holds one chunk at a time and every head walks the pattern again).
template <typename VT, bool VEC, bool COL, typename ARGS>
__device__ __forceinline__ void bwd_hub_head(const ARGS &A, const bool first, const size_t r, const int rl, const int t0,
                                             const int rem0, VT *a, VT *b, int *cl, VT *red, VT *red4)
{
    const int tid = (int)threadIdx.x;
    const bool staged = rl <= AT_STAGE; // (uniform over the workgroup, as every loop bound and barrier below)
    if constexpr (COL) {
        auto fill = [&](const int base, const int n) {
            for (int jj = tid; jj < n; jj += AT_BLOCK) {
                const int i = first || !staged ? A.col[att_storage(A, t0, rem0, base + jj)] : cl[jj];
                const VT av = bwd_value<VT>(A, t0, rem0, base + jj);
                VT p, ds;
                bwd_entry_col<VT, VEC>(A, (size_t)(uint32_t)i, r, av, bwd_drop_g<VT>(A, t0, rem0, base + jj), p, ds);
                a[jj] = p;
                b[jj] = ds;
                cl[jj] = i;
            }
        };
        if (staged)
            fill(0, rl);
        if (A.dV)
            bwd_hub_acc<VT>(rl, staged, fill, a, cl, A.dO, A.lddo, A.d, A.dV + r * A.lddv, red);
        if constexpr (ARGS::GAT) {
            if (A.dK)
                gat_hub_acc<VT, true, false>(rl, staged, fill, b, cl, A.Q, A.ldq, A.K + r * A.ldk, A.gat.a, A.gat.ns, A.k,
                                             A.dK + r * A.lddk, nullptr, red);
        } else if (A.dK)
            bwd_hub_acc<VT>(rl, staged, fill, b, cl, A.Q, A.ldq, A.k, A.dK + r * A.lddk, red);
    } else {
        VT mx = neg_inf<VT>();
        for (int j = tid; j < rl; j += AT_BLOCK) {
            const int cj = first || !staged ? A.col[att_storage(A, t0, rem0, j)] : cl[j];
            const VT av = bwd_value<VT>(A, t0, rem0, j);
            VT s, dp;
            bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)cj, av, bwd_drop_g<VT>(A, t0, rem0, j), s, dp);
            if (staged) {
                a[j] = s;
                b[j] = dp;
                cl[j] = cj;
            }
            mx = max_vt(mx, s);
        }
        mx = block_combine<VT, true>(wave_max(mx), red4);
        VT z = (VT)0;
        for (int j = tid; j < rl; j += AT_BLOCK) { // (a lane reads back what it stored itself, here and below)
            VT s;
            if (staged) {
                s = a[j];
            } else {
                const int cj = A.col[att_storage(A, t0, rem0, j)];
                const VT av = bwd_value<VT>(A, t0, rem0, j);
                s = bwd_score<VT, VEC>(A, r, (size_t)(uint32_t)cj, av);
            }
            const VT w = exp_vt(s - mx);
            if (staged)
                a[j] = w;
            z += w;
        }
        const VT rinv = (VT)1 / block_combine<VT, false>(wave_sum(z), red4);
        VT dsum = (VT)0;
        for (int j = tid; j < rl; j += AT_BLOCK) {
            VT w, dp;
            if (staged) {
                w = a[j];
                dp = b[j];
            } else {
                const int cj = A.col[att_storage(A, t0, rem0, j)];
                const VT av = bwd_value<VT>(A, t0, rem0, j);
                VT s;
                bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)cj, av, bwd_drop_g<VT>(A, t0, rem0, j), s, dp);
                w = exp_vt(s - mx);
            }
            const VT p = w * rinv;
            const VT pg = p * dp;
            if (staged)
                a[j] = p;
            dsum += pg;
        }
        const VT D = block_combine<VT, false>(wave_sum(dsum), red4);
        if (staged)
            for (int j = tid; j < rl; j += AT_BLOCK) {
                const VT ds = a[j] * (b[j] - D);
                bwd_store_ds(A, t0, rem0, j, ds);
                a[j] = bwd_coef(A, ds);
            }
        if constexpr (ARGS::BIASED) {
            if (!staged && A.dS) // (beyond the stage ds exists only inside dQ's chunk refills: one more sweep writes dS, the same bits)
                for (int j = tid; j < rl; j += AT_BLOCK) {
                    const int cj = A.col[att_storage(A, t0, rem0, j)];
                    const VT av = bwd_value<VT>(A, t0, rem0, j);
                    VT s, dp;
                    bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)cj, av, bwd_drop_g<VT>(A, t0, rem0, j), s, dp);
                    const VT p = exp_vt(s - mx) * rinv;
                    bwd_store_ds(A, t0, rem0, j, p * (dp - D));
                }
        }
        if (A.work && tid == 0) {
            VT *wk = A.work + (size_t)A.ws * r;
            wk[0] = mx;
            wk[1] = rinv;
            wk[2] = D;
        }
        auto fill = [&](const int base, const int n) {
            for (int jj = tid; jj < n; jj += AT_BLOCK) {
                const int cj = A.col[att_storage(A, t0, rem0, base + jj)];
                const VT av = bwd_value<VT>(A, t0, rem0, base + jj);
                VT s, dp;
                bwd_entry<VT, VEC>(A, r, (size_t)(uint32_t)cj, av, bwd_drop_g<VT>(A, t0, rem0, base + jj), s, dp);
                const VT p = exp_vt(s - mx) * rinv;
                a[jj] = bwd_coef(A, p * (dp - D));
                cl[jj] = cj;
            }
        };
        if constexpr (ARGS::GAT) {
            if (A.dQ || A.dAr)
                gat_hub_acc<VT, false, true>(rl, staged, fill, a, cl, A.K, A.ldk, A.Q + r * A.ldq, A.gat.a, A.gat.ns, A.k,
                                             A.dQ ? A.dQ + r * A.lddq : nullptr, A.dAr ? A.dAr + r * A.lddar : nullptr, red);
            else
                __syncthreads();
        } else if (A.dQ)
            bwd_hub_acc<VT>(rl, staged, fill, a, cl, A.K, A.ldk, A.k, A.dQ + r * A.lddq, red);
        else
            __syncthreads(); // (the stage is free for the next head or hub line)
    }
}

template <typename VT, bool VEC, bool COL, typename ARGS>
__device__ __forceinline__ void bwd_hub_line(const ARGS &A, const size_t r, const int rl, const int t0, const int rem0, VT *a,
                                             VT *b, int *cl, VT *red, VT *red4, const int h0, const int h1)
{
    for (int h = h0; h < h1; h++) // (uniform)
        bwd_hub_head<VT, VEC, COL>(bwd_head(A, h), h == h0, r, rl, t0, rem0, a, b, cl, red, red4);
}

// The kernels' body: the LDS (a, b, cl: the stage; red, red4: the reductions; hub_n, hub_row: the list of the workgroup's hub
// lines), the three line classes in turn.  MH: the packed multi-head call (blockIdx.y owns a contiguous group of heads); otherwise
// exactly one head, known at compile time.  A macro, not a function, for csr5_attention_kern.h's reason: the plain kernels keep,
// instruction for instruction, the code they had.
#define CSR5_ATTENTION_BWD_KERNEL_BODY(MH)                                                                                             \
    __shared__ VT a[AT_STAGE];                                                                                                         \
    __shared__ VT b[AT_STAGE];                                                                                                         \
    __shared__ int cl[AT_STAGE];                                                                                                       \
    __shared__ VT red[AT_BLOCK];                                                                                                       \
    __shared__ VT red4[AT_WAVES];                                                                                                      \
    __shared__ int hub_n;                                                                                                              \
    __shared__ int hub_row[AT_BLOCK];                                                                                                  \
    if (threadIdx.x == 0)                                                                                                              \
        hub_n = 0;                                                                                                                     \
    __syncthreads();                                                                                                                   \
                                                                                                                                       \
    int h0 = 0, h1 = 1;                                                                                                                \
    if constexpr (MH) {                                                                                                                \
        h0 = (int)blockIdx.y * A.hper;                                                                                                 \
        h1 = A.heads - h0 < A.hper ? A.heads : h0 + A.hper;                                                                            \
    }                                                                                                                                  \
    const int wave = (int)(threadIdx.x >> 6);                                                                                          \
    const long long row0 = (long long)blockIdx.x * AT_BLOCK + wave * OMEGA; /* the wavefront's first line */                           \
    const long long r = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;                                                                \
    int first = 0, len = -1, t0 = 0, rem0 = 0;                                                                                         \
    if (r < A.lines) {                                                                                                                 \
        first = A.row_ptr[r];                                                                                                          \
        len = A.row_ptr[r + 1] - first;                                                                                                \
        len = len < 0 ? 0 : len;                                                                                                       \
        t0 = (int)((unsigned)first / (unsigned)A.T);                                                                                   \
        rem0 = first - t0 * A.T;                                                                                                       \
    }                                                                                                                                  \
    bwd_short<VT, VEC, COL>(A, row0, len, t0, rem0, h0, h1);                                                                           \
                                                                                                                                       \
    unsigned long long todo = __ballot(len > AT_G && len <= AT_WAVE_ROW);                                                              \
    while (todo) {                                                                                                                     \
        const int src = __builtin_ctzll(todo);                                                                                         \
        todo &= todo - 1;                                                                                                              \
        bwd_wave_line<VT, VEC, COL>(A, (size_t)(row0 + src), __builtin_amdgcn_readlane(len, src), __builtin_amdgcn_readlane(t0, src),  \
                                    __builtin_amdgcn_readlane(rem0, src), a + wave * AT_WAVE_ROW, b + wave * AT_WAVE_ROW,              \
                                    cl + wave * AT_WAVE_ROW, h0, h1);                                                                  \
    }                                                                                                                                  \
                                                                                                                                       \
    if (len > AT_WAVE_ROW)                                                                                                             \
        hub_row[atomicAdd(&hub_n, 1)] = (int)threadIdx.x; /* (an integer counter in LDS: the order of the list decides no bit) */      \
    __syncthreads(); /* (and every wavefront is done with its share of the stage) */                                                   \
    const int hubs = __builtin_amdgcn_readfirstlane(hub_n);                                                                            \
    for (int i = 0; i < hubs; i++) { /* (uniform over the workgroup: the barriers inside are reached by all) */                        \
        const long long hr = (long long)blockIdx.x * AT_BLOCK + __builtin_amdgcn_readfirstlane(hub_row[i]);                            \
        const int ra = __builtin_amdgcn_readfirstlane(A.row_ptr[hr]);                                                                  \
        const int rl = __builtin_amdgcn_readfirstlane(A.row_ptr[hr + 1]) - ra;                                                         \
        const int ht0 = (int)((unsigned)ra / (unsigned)A.T);                                                                           \
        bwd_hub_line<VT, VEC, COL>(A, (size_t)hr, rl, ht0, ra - ht0 * A.T, a, b, cl, red, red4, h0, h1);                               \
    }

template <typename VT, bool VEC, bool COL, bool MH>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd(const AttBwdArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(MH)
}

// the biased call is always the packed one (heads = 1 is a group of one head)
template <typename VT, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd_biased(const AttBwdBiasArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// the edge-biased call likewise
template <typename VT, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd_edge(const AttBwdEdgeArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// the additive score likewise.  VEC: the dp chain's 16-byte loads of dO and V; the score takes element loads
template <typename VT, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd_gat(const AttBwdGatArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// the dropped calls: the edge call's and the additive one's kernels on their derived argument structs
template <typename VT, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd_drop(const AttBwdDropArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}
template <typename VT, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_bwd_drop_gat(const AttBwdDropGatArgs<VT> A)
{
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// 16-bit operands and outputs, float arithmetic: always the packed, edge-biased call.  6 waves per SIMD are
// k_attention_bwd_edge<float, ..>'s: left to itself the compiler widens a whole 32-byte block of bf16 ahead of the chain and takes 81
// (row kernel) and 82 (column kernel) registers with 16-byte loads, which are 5 waves
#if defined(__HIP__)
#define CSR5_ATT_BWD_LOWP_WAVES __attribute__((amdgpu_waves_per_eu(6)))
#else // (the host emulation compiles this header as plain C++, where no function is a kernel)
#define CSR5_ATT_BWD_LOWP_WAVES
#endif
template <typename ST, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) CSR5_ATT_BWD_LOWP_WAVES k_attention_bwd_lowp(const AttBwdLowpArgs<ST> A)
{
    using VT = float;
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// the dropped 16-bit call: k_attention_bwd_lowp on its derived argument struct, under the same 6-wave attribute.  Its chains take a
// 32-byte block in halves where ST is bf16 (bwd_halves, att_score's HALVES): with the whole block widened next to the hash's live
// words the bf16 kernels with 16-byte loads had 16 (row kernel) and 28 (column kernel) bytes of scratch per lane
template <typename ST, bool VEC, bool COL>
__global__ void __launch_bounds__(AT_BLOCK) CSR5_ATT_BWD_LOWP_WAVES k_attention_bwd_lowp_drop(const AttBwdLowpDropArgs<ST> A)
{
    using VT = float;
    CSR5_ATTENTION_BWD_KERNEL_BODY(true)
}

// the kernels of an argument struct, as overloads (csr5_attention_kern.h attention_enqueue).  COL: the column kernel
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd<VT, VEC, COL, MH>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdBiasArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_biased<VT, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdEdgeArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_edge<VT, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdGatArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_gat<VT, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdDropArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_drop<VT, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename VT>
static void attention_bwd_enqueue(const AttBwdDropGatArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_drop_gat<VT, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}

template <bool VEC, bool COL, bool MH, typename ST>
static void attention_bwd_enqueue(const AttBwdLowpArgs<ST> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_lowp<ST, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool COL, bool MH, typename ST>
static void attention_bwd_enqueue(const AttBwdLowpDropArgs<ST> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_bwd_lowp_drop<ST, VEC, COL>), grid, dim3(AT_BLOCK), 0, s, A);
}

// the pattern walked and the head groups of one side's launch.  groups: the head groups over grid.y, 0 for the rule
// (att_heads_per_group of this side's line count)
template <typename ARGS>
static void attention_bwd_fill(ARGS &A, const Geometry &g, const DeviceArrays &d, const int groups)
{
    A.lines = g.m;
    A.hper = groups > 0 ? (A.heads + groups - 1) / groups : att_heads_per_group(g.m, A.heads);
    A.sigma = g.sigma > 0 ? g.sigma : 1;
    A.T = g.tile_elems > 0 ? g.tile_elems : OMEGA;
    A.tiles = g.p > 1 ? g.p - 1 : 0;
    A.recip = (1u << 20) / (unsigned)A.sigma + 1u;
    A.row_ptr = d.row_ptr;
    A.col = d.col;
    A.tile_ptr = d.tile_ptr;
}

// 16-byte loads: every head's slice of every row of Q, K, V and dO starts on a 16-byte boundary (a chain shorter than one block
// of 32 bytes takes element loads anyway)
template <typename VT>
static bool attention_bwd_vec(int heads, int k, int dcols, const void *Q, int ldq, const void *K, int ldk, const void *V, int ldv,
                              const void *dO, int lddo)
{
    bool vec = heads == 1 || (((size_t)k * sizeof(VT)) % 16 == 0 && ((size_t)dcols * sizeof(VT)) % 16 == 0);
    const void *ptrs[4] = {Q, K, V, dO};
    const int lds[4] = {ldq, ldk, ldv, lddo};
    for (int i = 0; i < 4; i++)
        vec = vec && reinterpret_cast<uintptr_t>(ptrs[i]) % 16 == 0 && ((size_t)lds[i] * sizeof(VT)) % 16 == 0;
    return vec;
}

// one side's launch on the pattern (g, d) it walks; A: the call's fields and this side's outputs; map: null on the row side
template <bool COL, typename VT, typename ARGS>
static hipError_t attention_bwd_side(const Geometry &g, const DeviceArrays &d, ARGS A, const uint32_t *map, const AttBwdCall &c,
                                     hipStream_t s)
{
    if (g.m <= 0 || A.heads <= 0)
        return hipSuccess;
    attention_bwd_fill(A, g, d, c.groups);
    if constexpr (ARGS::BIASED)
        att_set_bias(A.bias, d, map, c);
    bool vec;
    if constexpr (ARGS::GAT) // (only the dp chain over dO and V takes 16-byte loads: Q and K need no alignment)
        vec = attention_bwd_vec<typename ARGS::ST>(c.heads, 0, c.d, c.V, c.ldv, c.V, c.ldv, c.V, c.ldv, c.dO, c.lddo);
    else
        vec = attention_bwd_vec<typename ARGS::ST>(c.heads, c.k, c.d, c.Q, c.ldq, c.K, c.ldk, c.V, c.ldv, c.dO, c.lddo);
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    if (A.heads == 1) {
        const dim3 grid(blocks);
        if (vec)
            attention_bwd_enqueue<true, COL, false>(A, grid, s);
        else
            attention_bwd_enqueue<false, COL, false>(A, grid, s);
    } else {
        const dim3 grid(blocks, (unsigned)((A.heads + A.hper - 1) / A.hper));
        if (vec)
            attention_bwd_enqueue<true, COL, true>(A, grid, s);
        else
            attention_bwd_enqueue<false, COL, true>(A, grid, s);
    }
    return hipGetLastError();
}

// The launcher of every backward unit: ARGS is the unit's argument struct (AttBwd..Args<VT>), which decides the kernels
// (attention_bwd_enqueue) and the bias fields (att_set_bias); VT: the type computed in and of the workspace, ARGS::ST the operands'
// and the outputs'.  g / d: the parent's pattern (the row kernel); c.gt / c.dt (edge: and c.map): the transposed companion's (the
// column kernel, only when dK or dV is wanted).  The row kernel runs when dQ or dS is wanted or the column kernel needs the
// workspace; dS is the row side's alone.
template <typename VT, typename ARGS>
hipError_t attention_bwd_launch(const Geometry &g, const DeviceArrays &d, const AttBwdCall &c, hipStream_t s)
{
    using ST = typename ARGS::ST;
    ARGS A{};
    A.k = c.k;
    A.d = c.d;
    A.heads = c.heads;
    A.ws = 4 * c.heads;
    A.Q = (const ST *)c.Q;
    A.K = (const ST *)c.K;
    A.V = (const ST *)c.V;
    A.dO = (const ST *)c.dO;
    A.ldq = c.ldq;
    A.ldk = c.ldk;
    A.ldv = c.ldv;
    A.lddo = c.lddo;
    A.lddq = c.lddq;
    A.lddk = c.lddk;
    A.lddv = c.lddv;
    void *dS = nullptr;
    if constexpr (ARGS::BIASED)
        dS = c.dS;
    void *dAr = nullptr; // (the additive score's second row-side output: wanted as dQ is)
    if constexpr (ARGS::GAT) {
        att_set_gat(A.gat, c);
        dAr = c.k > 0 ? c.dAr : nullptr;
    }
    if constexpr (ARGS::DROP)
        att_set_drop(A.drop, c);
    const bool column = c.gt && c.dt && (!ARGS::EDGE || c.map) && (c.dK || c.dV);
    hipError_t e = hipSuccess;
    if (c.dQ || dS || column || dAr) {
        ARGS R = A;
        R.dQ = c.k > 0 ? (ST *)c.dQ : nullptr;
        R.work = column ? (VT *)c.work : nullptr;
        if constexpr (ARGS::BIASED) {
            R.dS = (ST *)dS;
            R.ldds = c.ldds;
        }
        if constexpr (ARGS::GAT) {
            R.dAr = (ST *)dAr;
            R.lddar = c.lddar;
        }
        if (R.dQ || R.work || dS || dAr)
            e = attention_bwd_side<false, VT>(g, d, R, nullptr, c, s);
    }
    if (e == hipSuccess && column) {
        ARGS C = A;
        C.dK = c.k > 0 ? (ST *)c.dK : nullptr;
        C.dV = c.d > 0 ? (ST *)c.dV : nullptr;
        C.work = (VT *)c.work;
        if (C.dK || C.dV)
            e = attention_bwd_side<true, VT>(*c.gt, *c.dt, C, c.map, c, s);
    }
    return e;
}

} // namespace csr5
