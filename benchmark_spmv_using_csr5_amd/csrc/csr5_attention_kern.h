// csr5_attention_kern.h -- the kernel templates of the one-pass attention on the pattern and their typed launcher; the contract is
// written out at the head of csr5_attention.hip.  Two translation units instantiate them: csr5_attention.hip the plain entry
// points (csr5hip_attention, csr5hip_mha; AttArgs), csr5_attention_bias.hip the biased one (csr5hip_mha_biased; AttBiasArgs),
// csr5_attention_edge.hip the edge-biased one (csr5hip_mha_edge_bias; AttEdgeArgs: ARGS::EDGE, the bias from a caller's (nnz, heads)
// tensor at the entry's CSR rank instead of from the handle's values).
// csr5_attention_lowp.hip instantiates them a fourth time with operands STORED in bf16 or fp16 and float arithmetic (csr5hip_mha_lowp;
// AttLowpArgs, k_attention_lowp): ARGS::ST is the type behind the operand pointers, VT the type of everything computed.  Where
// ST == VT the casts between them are no operation, and the kernels of the other units are, instruction for instruction, what they
// were without them (scripts/compare_attention_asm.py).
// THE BIAS IS A COMPILE-TIME PROPERTY OF THE ARGUMENT STRUCT (ARGS::BIASED): the plain instantiations carry no bias argument,
// no branch and no load for it -- their kernarg block and their code are those of the templates without it.
// csr5_attention_drop_lowp.hip: the 16-bit call with the dropout mask (csr5hip_dropout_mha_lowp; AttLowpDropArgs, k_attention_lowp_drop).
// Include it after `#pragma clang fp contract(off)`; gfx950 (wave64) only.
#pragma once

#include "csr5_attention_dev.h"

namespace csr5 {

template <typename VT>
struct AttArgs {
    static constexpr bool BIASED = false;
    static constexpr bool EDGE = false; // (with BIASED: the bias is AttEdgeBias, read at the entry's CSR rank)
    static constexpr bool GAT = false;  // (with EDGE: the additive score of AttGatArgs in place of the dot product)
    static constexpr bool DROP = false; // (with EDGE: the dropout mask of AttDropArgs / AttDropGatArgs on the weights)
    using ST = VT;                      // the type Q, K, V and O are stored in (AttLowpArgs: another one than the arithmetic's)
    int m, k, d;
    int heads, hper;     // heads of the packed operands; heads of one workgroup (blockIdx.y owns heads y hper .. y hper + hper - 1)
    int T, sigma, tiles; // tile_elems, sigma, p - 1 (tiles in tile order; beyond them the CSR tail)
    unsigned recip;      // sigma's reciprocal in 20 fractional bits, rounded up (csr5_refresh.hip refresh_div)
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const VT *Q, *K, *V;
    VT *O;
    int ldq, ldk, ldv, ldo;
};

// csr5hip_mha_biased: s = fma(qk, c, slope_h * a_e), a_e the handle's value of the entry (att_bias_score)
template <typename VT>
struct AttBiasArgs : AttArgs<VT> {
    static constexpr bool BIASED = true;
    AttBias<VT> bias;
};

// csr5hip_mha_edge_bias: s = fma(qk, c, B[e * ldb + h]), e the entry's CSR rank (att_edge_value); the handle's values are not read
template <typename VT>
struct AttEdgeArgs : AttArgs<VT> {
    static constexpr bool BIASED = true;
    static constexpr bool EDGE = true;
    AttEdgeBias<VT> bias;
};

// csr5hip_gat (csr5_attention_gat.hip): the edge call with z = sum_c a[h, c] LeakyReLU(Q[i, h, c] + K[j, h, c]) (att_gat_z) in the
// dot product's place: s = fma(z, c, B[e * ldb + h]).  Everything after the score is the edge call's
template <typename VT>
struct AttGatArgs : AttEdgeArgs<VT> {
    static constexpr bool GAT = true;
    AttGat<VT> gat;
};

// csr5hip_dropout_mha (csr5_attention_drop.hip) and csr5hip_dropout_gat (csr5_attention_drop_gat.hip): the edge call and the additive
// one with a seeded dropout mask on the weights (csr5_attention_dev.h AttDrop).  M, w and Z are the undropped call's -- the softmax is
// over all stored entries --; the weight that enters the product is keep ? w : +0, and the row's factor is rinv * cd, one
// multiplication per row and head.  With thr = 0 and cd = 1 every bit is the undropped call's.
template <typename VT>
struct AttDropArgs : AttEdgeArgs<VT> {
    static constexpr bool DROP = true;
    AttDrop<VT> drop;
};
template <typename VT>
struct AttDropGatArgs : AttGatArgs<VT> {
    static constexpr bool DROP = true;
    AttDrop<VT> drop;
};

// the weight of head h of the entry of rank e that enters the product: w, dropped +0
template <typename VT, typename ARGS>
__device__ __forceinline__ VT att_dropped(const ARGS &A, const size_t e, const int h, const VT w)
{
    return att_drop_keep(A.drop.key, e, h) ? w : (VT)0;
}

// the additive score's z of an entry of head h: att_gat_z on that head's k values of a
template <typename VT, typename ARGS>
__device__ __forceinline__ VT att_gat_chain(const ARGS &A, const int h, const VT *q, const VT *kr)
{
    return att_gat_z<VT>(q, kr, A.gat.a ? A.gat.a + (size_t)h * A.k : nullptr, A.gat.ns, A.k);
}

// csr5hip_mha_lowp (csr5_attention_lowp.hip): AttEdgeArgs<float>'s call with Q, K, V, B and O STORED in ST (bf16 or fp16).  The
// arithmetic is float: the templates below widen an operand where they load it and round once where they store O, and are
// otherwise the float instantiation's, statement for statement -- the result is the rounding of the float call's on the widened
// operands.  A struct of its own: the existing ones keep their names and layouts, and their kernels their code.
template <typename ST_>
struct AttLowpArgs {
    static constexpr bool BIASED = true;
    static constexpr bool EDGE = true;
    static constexpr bool GAT = false;
    static constexpr bool DROP = false;
    using ST = ST_;
    int m, k, d;
    int heads, hper;
    int T, sigma, tiles;
    unsigned recip;
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const ST *Q, *K, *V;
    ST *O;
    int ldq, ldk, ldv, ldo;
    AttEdgeBiasLowp<ST> bias;
};

// csr5hip_dropout_mha_lowp (csr5_attention_drop_lowp.hip): AttDropArgs<float>'s call on operands stored in ST -- the 16-bit call with
// the dropout mask on the float weights, derived as AttDropArgs is from the edge struct.  cd is float, as everything computed
template <typename ST_>
struct AttLowpDropArgs : AttLowpArgs<ST_> {
    static constexpr bool DROP = true;
    AttDrop<float> drop;
};

// ---- rows of at most 16 entries (empty rows included): 16 lanes per row, 4 rows of the wavefront per pass ------------------
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void att_short(const ARGS &A, const long long row0, const int len, const int t0, const int rem0, const int h0,
                                          const int h1)
{
    constexpr int G = AT_G, ROWS = OMEGA / G;
    const int lane = threadIdx.x & (OMEGA - 1);
    const int sub = lane / G, pos = lane % G;
    const unsigned long long cls = __ballot(len >= 0 && len <= G); // (len = -1: no such row)
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
        int cj = 0; // the lane's column (and, biased, its value; edge-biased, its CSR rank): loaded once, kept across the heads
        VT av = (VT)0;
        size_t er = 0;
        if (act) {
            const size_t st = att_storage(A, rt0, rrem, pos);
            cj = A.col[st];
            if constexpr (ARGS::EDGE)
                er = (size_t)rt0 * A.T + (size_t)rrem + (size_t)pos;
            else if constexpr (ARGS::BIASED)
                av = A.bias.val[st];
        }
        for (int h = h0; h < h1; h++) { // (uniform)
            const typename ARGS::ST *Vh = A.V + (size_t)h * A.d;
            typename ARGS::ST *Oh = A.O + (size_t)h * A.d;
            VT s = neg_inf<VT>();
            if (act) {
                if constexpr (ARGS::GAT)
                    s = att_gat_chain<VT>(A, h, A.Q + r * A.ldq + (size_t)h * A.k,
                                          A.K + (size_t)(uint32_t)cj * A.ldk + (size_t)h * A.k);
                else
                    s = att_score<VT, VEC>(A.Q + r * A.ldq + (size_t)h * A.k, A.K + (size_t)(uint32_t)cj * A.ldk + (size_t)h * A.k,
                                           A.k);
                if constexpr (ARGS::EDGE)
                    s = att_bias_score(A.bias, h, s, att_edge_value(A.bias, er, h));
                else if constexpr (ARGS::BIASED)
                    s = att_bias_score(A.bias, h, s, av);
            }
            const VT mx = group_max<G>(s);
            VT w = act ? exp_vt(s - mx) : (VT)0;
            VT rinv = (VT)1 / group_sum<G>(w);
            if constexpr (ARGS::DROP) { // (after Z: the softmax is over all stored entries)
                w = act ? att_dropped(A, er, h, w) : (VT)0;
                rinv = rinv * A.drop.cd;
            }
            for (int cb = 0; cb < A.d; cb += G) { // (uniform)
                const int c = cb + pos;
                VT acc = (VT)0;
                for (int e = 0; e < G; e++) {
                    if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                        break;
                    const VT we = __shfl(w, sub * G + e, OMEGA);
                    const int je = __shfl(cj, sub * G + e, OMEGA);
                    if (rowok && e < rl && c < A.d)
                        acc = fma_vt(we, (VT)Vh[(size_t)(uint32_t)je * A.ldv + c], acc);
                }
                if (rowok && c < A.d)
                    Oh[r * A.ldo + c] = att_stored<typename ARGS::ST>(rl > 0 ? acc * rinv : (VT)0);
            }
        }
    }
}

// ---- a row of 17 .. 512 entries: one wavefront; sc / cl: the wavefront's 512 staged scores (then weights) and columns ------
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void att_wave_row(const ARGS &A, const size_t r, const int rl, const int t0, const int rem0, VT *sc, int *cl,
                                             const int h0, const int h1)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int h = h0; h < h1; h++) { // (uniform) cl is staged by the first head and kept; sc is refilled per head
        const typename ARGS::ST *q = A.Q + r * A.ldq + (size_t)h * A.k;
        const typename ARGS::ST *Kh = A.K + (size_t)h * A.k;
        VT mx = neg_inf<VT>();
        for (int j = lane; j < rl; j += OMEGA) { // (a lane reads back the columns it stored itself)
            int cj;
            if (h == h0) {
                cj = A.col[att_storage(A, t0, rem0, j)];
                cl[j] = cj;
            } else {
                cj = cl[j];
            }
            VT s;
            if constexpr (ARGS::GAT)
                s = att_gat_chain<VT>(A, h, q, Kh + (size_t)(uint32_t)cj * A.ldk);
            else
                s = att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k);
            if constexpr (ARGS::EDGE) // (the bias is read from the entry's rank by every head: it is not staged either)
                s = att_bias_score(A.bias, h, s, att_edge_value(A.bias, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j, h));
            else if constexpr (ARGS::BIASED) // (the value is read again from the column's index by every head: it is not staged)
                s = att_bias_score(A.bias, h, s, A.bias.val[att_storage(A, t0, rem0, j)]);
            sc[j] = s;
            mx = max_vt(mx, s);
        }
        mx = wave_max(mx);
        VT z = (VT)0;
        for (int j = lane; j < rl; j += OMEGA) { // (a lane reads back what it stored itself)
            const VT w = exp_vt(sc[j] - mx);
            if constexpr (ARGS::DROP)
                sc[j] = att_dropped(A, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j, h, w);
            else
                sc[j] = w;
            z += w;
        }
        VT rinv = (VT)1 / wave_sum(z);
        if constexpr (ARGS::DROP)
            rinv = rinv * A.drop.cd;
        att_wave_sync();
        for (int cb = 0; cb < A.d; cb += OMEGA) {
            const int wb = A.d - cb < OMEGA ? A.d - cb : OMEGA;
            const int C = att_pow2(wb), S = OMEGA / C;
            const int slot = lane / C, cc = lane & (C - 1);
            VT acc = (VT)0;
            if (cc < wb) {
                const typename ARGS::ST *v = A.V + (size_t)h * A.d + cb + cc;
#pragma unroll 4
                for (int e = slot; e < rl; e += S)
                    acc = fma_vt(sc[e], (VT)v[(size_t)(uint32_t)cl[e] * A.ldv], acc);
            }
            for (int off = C; off < OMEGA; off <<= 1) // (uniform; adjacent slots first)
                acc += __shfl_xor(acc, off, OMEGA);
            if (slot == 0 && cc < wb)
                A.O[r * A.ldo + (size_t)h * A.d + cb + cc] = att_stored<typename ARGS::ST>(acc * rinv);
        }
        att_wave_sync(); // (the next head's and the next row's scores stay behind these reads)
    }
}

// ---- a row beyond 512 entries: the workgroup; sc / cl: the AT_STAGE staged entries, red: AT_BLOCK values, red4: AT_WAVES -----
// One head h of the row: q, Kh, Vh, o are that head's slices.  first: the head that stages cl of a row of at most AT_STAGE entries;
// the later heads take the columns from there.  (Beyond AT_STAGE entries the stage holds one chunk at a time and every head
// walks the pattern again: keeping the chunk across the heads would take 4 accumulators per head and lane.)
template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void att_hub_head(const ARGS &A, const int h, const typename ARGS::ST *q, const typename ARGS::ST *Kh,
                                             const typename ARGS::ST *Vh, typename ARGS::ST *o_row, const bool first,
                                             const int rl, const int t0, const int rem0, VT *sc, int *cl, VT *red, VT *red4)
{
    const int tid = (int)threadIdx.x;
    const bool staged = rl <= AT_STAGE; // (uniform over the workgroup, as every loop bound and barrier below)
    VT mx = neg_inf<VT>();
    for (int j = tid; j < rl; j += AT_BLOCK) { // (a lane reads back the columns it stored itself)
        int cj;
        if (first || !staged)
            cj = A.col[att_storage(A, t0, rem0, j)];
        else
            cj = cl[j];
        VT s;
        if constexpr (ARGS::GAT)
            s = att_gat_chain<VT>(A, h, q, Kh + (size_t)(uint32_t)cj * A.ldk);
        else
            s = att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k);
        if constexpr (ARGS::EDGE)
            s = att_bias_score(A.bias, h, s, att_edge_value(A.bias, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j, h));
        else if constexpr (ARGS::BIASED)
            s = att_bias_score(A.bias, h, s, A.bias.val[att_storage(A, t0, rem0, j)]);
        if (staged) {
            sc[j] = s;
            if (first)
                cl[j] = cj;
        }
        mx = max_vt(mx, s);
    }
    mx = block_combine<VT, true>(wave_max(mx), red4);
    VT z = (VT)0;
    if (staged) {
        for (int j = tid; j < rl; j += AT_BLOCK) { // (a lane reads back what it stored itself)
            const VT w = exp_vt(sc[j] - mx);
            if constexpr (ARGS::DROP)
                sc[j] = att_dropped(A, (size_t)t0 * A.T + (size_t)rem0 + (size_t)j, h, w);
            else
                sc[j] = w;
            z += w;
        }
    }
    VT rinv = (VT)0;
    for (int cg = 0; cg < A.d; cg += OMEGA * AT_HUB_BLOCKS) {
        VT acc[AT_HUB_BLOCKS];
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++)
            acc[b] = (VT)0;
        for (int base = 0; base < rl; base += AT_STAGE) {
            const int n = rl - base < AT_STAGE ? rl - base : AT_STAGE;
            if (!staged) {
                __syncthreads(); // (the stage is free: the previous chunk has been read)
                for (int jj = tid; jj < n; jj += AT_BLOCK) {
                    const size_t st = att_storage(A, t0, rem0, base + jj);
                    const int cj = A.col[st];
                    VT s;
                    if constexpr (ARGS::GAT)
                        s = att_gat_chain<VT>(A, h, q, Kh + (size_t)(uint32_t)cj * A.ldk);
                    else
                        s = att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k);
                    if constexpr (ARGS::EDGE)
                        s = att_bias_score(A.bias, h, s,
                                           att_edge_value(A.bias, (size_t)t0 * A.T + (size_t)rem0 + (size_t)(base + jj), h));
                    else if constexpr (ARGS::BIASED)
                        s = att_bias_score(A.bias, h, s, A.bias.val[st]);
                    const VT w = exp_vt(s - mx);
                    if constexpr (ARGS::DROP)
                        sc[jj] = att_dropped(A, (size_t)t0 * A.T + (size_t)rem0 + (size_t)(base + jj), h, w);
                    else
                        sc[jj] = w;
                    cl[jj] = cj;
                    if (cg == 0)
                        z += w;
                }
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < AT_HUB_BLOCKS; b++) {
                const int cb = cg + b * OMEGA;
                if (cb < A.d) {
                    const int wb = A.d - cb < OMEGA ? A.d - cb : OMEGA;
                    const int C = att_pow2(wb), S = AT_BLOCK / C; // (AT_STAGE is a multiple of S: a chunk keeps j mod S)
                    const int slot = tid / C, cc = tid & (C - 1);
                    if (cc < wb) {
                        const typename ARGS::ST *v = Vh + cb + cc;
                        VT o = acc[b];
#pragma unroll 4
                        for (int e = slot; e < n; e += S)
                            o = fma_vt(sc[e], (VT)v[(size_t)(uint32_t)cl[e] * A.ldv], o);
                        acc[b] = o;
                    }
                }
            }
        }
        if (cg == 0) {
            rinv = (VT)1 / block_combine<VT, false>(wave_sum(z), red4);
            if constexpr (ARGS::DROP)
                rinv = rinv * A.drop.cd;
        }
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            const int cb = cg + b * OMEGA;
            if (cb < A.d) { // (uniform)
                const int wb = A.d - cb < OMEGA ? A.d - cb : OMEGA;
                const int C = att_pow2(wb);
                VT o = acc[b];
                for (int off = C; off < OMEGA; off <<= 1) // adjacent slots of the wavefront first ...
                    o += __shfl_xor(o, off, OMEGA);
                red[tid] = o;
                __syncthreads();
                if (tid < wb) // ... then (w0 + w1) + (w2 + w3); lane c < C of every wavefront holds column c
                    o_row[cb + tid] = att_stored<typename ARGS::ST>(
                        ((red[tid] + red[OMEGA + tid]) + (red[2 * OMEGA + tid] + red[3 * OMEGA + tid])) * rinv);
                __syncthreads(); // (red is free for the next block)
            }
        }
    }
    __syncthreads(); // (the stage is free for the next head or hub row)
}

template <typename VT, bool VEC, typename ARGS>
__device__ __forceinline__ void att_hub_row(const ARGS &A, const size_t r, const int rl, const int t0, const int rem0, VT *sc, int *cl,
                                            VT *red, VT *red4, const int h0, const int h1)
{
    for (int h = h0; h < h1; h++) // (uniform)
        att_hub_head<VT, VEC>(A, h, A.Q + r * A.ldq + (size_t)h * A.k, A.K + (size_t)h * A.k, A.V + (size_t)h * A.d,
                              A.O + r * A.ldo + (size_t)h * A.d, h == h0, rl, t0, rem0, sc, cl, red, red4);
}

// The kernels' body: the LDS (sc, cl: the stage; red, red4: the reductions; hub_n, hub_row: the list of the workgroup's hub rows),
// the three row classes in turn.  MH: the packed multi-head call (blockIdx.y owns a contiguous group of heads); otherwise exactly
// one head, known at compile time.  A MACRO, NOT A FUNCTION: the compiler allocates registers and schedules a body that reaches
// the kernel through one more inlined function differently, and the plain kernels keep, instruction for instruction, the code
// they had before the biased ones shared their templates.
#define CSR5_ATTENTION_KERNEL_BODY(MH)                                                                                             \
    __shared__ VT sc[AT_STAGE];                                                                                                    \
    __shared__ int cl[AT_STAGE];                                                                                                   \
    __shared__ VT red[AT_BLOCK];                                                                                                   \
    __shared__ VT red4[AT_WAVES];                                                                                                  \
    __shared__ int hub_n;                                                                                                          \
    __shared__ int hub_row[AT_BLOCK];                                                                                              \
    if (threadIdx.x == 0)                                                                                                          \
        hub_n = 0;                                                                                                                 \
    __syncthreads();                                                                                                               \
                                                                                                                                   \
    int h0 = 0, h1 = 1;                                                                                                            \
    if constexpr (MH) {                                                                                                            \
        h0 = (int)blockIdx.y * A.hper;                                                                                             \
        h1 = A.heads - h0 < A.hper ? A.heads : h0 + A.hper;                                                                        \
    }                                                                                                                              \
    const int wave = (int)(threadIdx.x >> 6);                                                                                      \
    const long long row0 = (long long)blockIdx.x * AT_BLOCK + wave * OMEGA; /* the wavefront's first row */                        \
    const long long r = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;                                                            \
    int a = 0, len = -1, t0 = 0, rem0 = 0;                                                                                         \
    if (r < A.m) {                                                                                                                 \
        a = A.row_ptr[r];                                                                                                          \
        len = A.row_ptr[r + 1] - a;                                                                                                \
        len = len < 0 ? 0 : len;                                                                                                   \
        t0 = (int)((unsigned)a / (unsigned)A.T);                                                                                   \
        rem0 = a - t0 * A.T;                                                                                                       \
    }                                                                                                                              \
    att_short<VT, VEC>(A, row0, len, t0, rem0, h0, h1);                                                                            \
                                                                                                                                   \
    unsigned long long todo = __ballot(len > AT_G && len <= AT_WAVE_ROW);                                                          \
    while (todo) {                                                                                                                 \
        const int src = __builtin_ctzll(todo);                                                                                     \
        todo &= todo - 1;                                                                                                          \
        att_wave_row<VT, VEC>(A, (size_t)(row0 + src), __builtin_amdgcn_readlane(len, src), __builtin_amdgcn_readlane(t0, src),    \
                              __builtin_amdgcn_readlane(rem0, src), sc + wave * AT_WAVE_ROW, cl + wave * AT_WAVE_ROW, h0, h1);     \
    }                                                                                                                              \
                                                                                                                                   \
    if (len > AT_WAVE_ROW)                                                                                                         \
        hub_row[atomicAdd(&hub_n, 1)] = (int)threadIdx.x; /* (an integer counter in LDS: the order of the list decides no bit) */  \
    __syncthreads(); /* (and every wavefront is done with its share of the stage) */                                               \
    const int hubs = __builtin_amdgcn_readfirstlane(hub_n);                                                                        \
    for (int i = 0; i < hubs; i++) { /* (uniform over the workgroup: the barriers inside are reached by all) */                    \
        const long long hr = (long long)blockIdx.x * AT_BLOCK + __builtin_amdgcn_readfirstlane(hub_row[i]);                        \
        const int ra = __builtin_amdgcn_readfirstlane(A.row_ptr[hr]);                                                              \
        const int rl = __builtin_amdgcn_readfirstlane(A.row_ptr[hr + 1]) - ra;                                                     \
        const int ht0 = (int)((unsigned)ra / (unsigned)A.T);                                                                       \
        att_hub_row<VT, VEC>(A, (size_t)hr, rl, ht0, ra - ht0 * A.T, sc, cl, red, red4, h0, h1);                                   \
    }

template <typename VT, bool VEC, bool MH>
__global__ void __launch_bounds__(AT_BLOCK) k_attention(const AttArgs<VT> A)
{
    CSR5_ATTENTION_KERNEL_BODY(MH)
}

// the biased call is always the packed one (heads = 1 is a group of one head)
template <typename VT, bool VEC>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_biased(const AttBiasArgs<VT> A)
{
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// the edge-biased call likewise
template <typename VT, bool VEC>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_edge(const AttEdgeArgs<VT> A)
{
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// the additive score likewise.  It takes element loads only, so there is one kernel per value type, whatever the launcher's VEC
template <typename VT>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_gat(const AttGatArgs<VT> A)
{
    constexpr bool VEC = false;
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// the dropped calls: the edge call's and the additive one's kernels on their derived argument structs
template <typename VT, bool VEC>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_drop(const AttDropArgs<VT> A)
{
    CSR5_ATTENTION_KERNEL_BODY(true)
}
template <typename VT>
__global__ void __launch_bounds__(AT_BLOCK) k_attention_drop_gat(const AttDropGatArgs<VT> A)
{
    constexpr bool VEC = false;
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// 16-bit operands, float arithmetic: always the packed, edge-biased call.  7 waves per SIMD are k_attention_edge<float, ..>'s: left to
// itself the compiler widens a whole 32-byte block of bf16 ahead of the chain and takes 75 registers (6 waves)
#if defined(__HIP__)
#define CSR5_ATT_LOWP_WAVES __attribute__((amdgpu_waves_per_eu(7)))
#else // (the host emulation compiles this header as plain C++, where no function is a kernel)
#define CSR5_ATT_LOWP_WAVES
#endif
template <typename ST, bool VEC>
__global__ void __launch_bounds__(AT_BLOCK) CSR5_ATT_LOWP_WAVES k_attention_lowp(const AttLowpArgs<ST> A)
{
    using VT = float;
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// the dropped 16-bit call: k_attention_lowp on its derived argument struct, under the same occupancy attribute
template <typename ST, bool VEC>
__global__ void __launch_bounds__(AT_BLOCK) CSR5_ATT_LOWP_WAVES k_attention_lowp_drop(const AttLowpDropArgs<ST> A)
{
    using VT = float;
    CSR5_ATTENTION_KERNEL_BODY(true)
}

// the kernels of an argument struct, as overloads, so that the launcher below is written once.  MH: only the plain call has a
// single-head instantiation; the others are always the packed call
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention<VT, VEC, MH>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttBiasArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_biased<VT, VEC>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttEdgeArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_edge<VT, VEC>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttGatArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_gat<VT>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttDropArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_drop<VT, VEC>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename VT>
static void attention_enqueue(const AttDropGatArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_drop_gat<VT>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename ST>
static void attention_enqueue(const AttLowpArgs<ST> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_lowp<ST, VEC>), grid, dim3(AT_BLOCK), 0, s, A);
}
template <bool VEC, bool MH, typename ST>
static void attention_enqueue(const AttLowpDropArgs<ST> &A, const dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_attention_lowp_drop<ST, VEC>), grid, dim3(AT_BLOCK), 0, s, A);
}

// the pattern, the operands and the head groups of a launch.  VT: the type the operands are stored in
template <typename VT, typename ARGS>
static void attention_fill(ARGS &A, const Geometry &g, const DeviceArrays &d, const AttCall &c)
{
    A.m = g.m;
    A.k = c.k;
    A.d = c.d;
    A.heads = c.heads;
    A.hper = c.groups > 0 ? (c.heads + c.groups - 1) / c.groups : att_heads_per_group(g.m, c.heads);
    A.sigma = g.sigma > 0 ? g.sigma : 1;
    A.T = g.tile_elems > 0 ? g.tile_elems : OMEGA;
    A.tiles = g.p > 1 ? g.p - 1 : 0;
    A.recip = (1u << 20) / (unsigned)A.sigma + 1u;
    A.row_ptr = d.row_ptr;
    A.col = d.col;
    A.tile_ptr = d.tile_ptr;
    A.Q = (const VT *)c.Q;
    A.K = (const VT *)c.K;
    A.V = (const VT *)c.V;
    A.O = (VT *)c.O;
    A.ldq = c.ldq;
    A.ldk = c.ldk;
    A.ldv = c.ldv;
    A.ldo = c.ldo;
}

// 16-byte loads: at least one whole block, and every head's slice of every row of Q and of K starts on a 16-byte boundary
template <typename VT>
static bool attention_vec(int heads, const void *Q, int ldq, const void *K, int ldk, int k)
{
    return k >= 32 / (int)sizeof(VT) && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(K) % 16 == 0 &&
           ((size_t)ldq * sizeof(VT)) % 16 == 0 && ((size_t)ldk * sizeof(VT)) % 16 == 0 &&
           (heads == 1 || ((size_t)k * sizeof(VT)) % 16 == 0);
}

// The launcher of every forward unit: ARGS is the unit's argument struct, which decides the kernels (attention_enqueue) and the
// bias fields (att_set_bias).  heads == 1 of the plain call is the single-head instantiation, on a grid without head groups.
template <typename ARGS>
hipError_t attention_launch(const Geometry &g, const DeviceArrays &d, const AttCall &c, hipStream_t s)
{
    using ST = typename ARGS::ST;
    if (g.m <= 0 || c.d <= 0 || c.heads <= 0)
        return hipSuccess;
    ARGS A;
    attention_fill<ST>(A, g, d, c);
    if constexpr (ARGS::BIASED)
        att_set_bias(A.bias, d, nullptr, c);
    if constexpr (ARGS::GAT)
        att_set_gat(A.gat, c);
    if constexpr (ARGS::DROP)
        att_set_drop(A.drop, c);
    bool vec = false; // (the additive score takes element loads: one kernel, whatever the alignment of Q and K)
    if constexpr (!ARGS::GAT)
        vec = attention_vec<ST>(c.heads, c.Q, c.ldq, c.K, c.ldk, c.k);
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    if (c.heads == 1) {
        const dim3 grid(blocks);
        if (vec)
            attention_enqueue<true, false>(A, grid, s);
        else
            attention_enqueue<false, false>(A, grid, s);
    } else {
        const dim3 grid(blocks, (unsigned)((c.heads + A.hper - 1) / A.hper));
        if (vec)
            attention_enqueue<true, true>(A, grid, s);
        else
            attention_enqueue<false, true>(A, grid, s);
    }
    return hipGetLastError();
}

} // namespace csr5
