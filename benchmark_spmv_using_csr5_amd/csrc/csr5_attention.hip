// csr5_attention.hip -- attention on the pattern in ONE pass (scores, softmax over the row, product with V) for gfx950 (wave64):
//
//     s_e     = Q[i, :] . K[j_e, :]              for the stored entries e of row i, in CSR order, j_e the column of entry e
//     O[i, c] = (sum_e exp(s_e - M_i) V[j_e, c]) / Z_i     M_i = max_e s_e,  Z_i = sum_e exp(s_e - M_i),  c < d
//
// Q is m x k, K is n x k, V is n x d, O is m x d, row-major with leading dimensions ldq / ldk / ldv / ldo.  Nothing of length nnz is
// written or read back: a row's scores and weights live in registers or LDS.  The kernel is row-oriented: bounds from row_ptr (as
// k_row_softmax), columns from the tile-ordered column_index through the rank -> storage map below.  It reads row_ptr, tile_ptr
// and column_index of the parent handle and NOTHING else of it: no values, no x, no descriptors, no slab structures, no kernel
// tables.  No workspace, no floating-point atomics, no scratch; one launch, enqueue-only.
//
// EVERY row of O is written in columns 0 .. d-1: a row without entries gets +0 (csr5hip_spmm leaves such rows alone), so the caller
// may pass uninitialised memory.  Columns d .. ldo-1 are never written.
//
// DEFINITION.  s_e is csr5hip_sddmm's chain, fma(Q[k-1], K[k-1], ... fma(Q[0], K[0], +0) ...), the same bits.  M is the exact
// maximum of the row's scores (NaN skipped by the maximum; it then poisons the sum).  w_e = exp(s_e - M): ONE subtraction, ONE
// exponential of the device library (exp / expf at full precision, subnormal results kept).  Z sums the w_e by the tree below.
// THE NORMALISATION COMES AFTER THE PRODUCT: acc_c = sum_e w_e V[j_e, c] accumulated by fused multiply-adds in the order below,
// then ONE reciprocal per row, r = 1 / Z (a correctly rounded division), and ONE multiplication per output, O[i, c] = acc_c * r.
// No running maximum is rescaled: M is known before the first exponential.  Nothing but the written-out FMAs is contracted.
//
// NON-FINITE values behave as the unfused chain sddmm -> row_softmax -> spmm: a -Inf score has weight +0; a row that holds a NaN
// score, holds a +Inf score (Inf - Inf) or only -Inf scores (-Inf - -Inf) has Z = NaN and is NaN in all d outputs; no other row
// is touched: a row is computed from its own entries only (padding lanes contribute +0 through a select).
//
// RANK -> STORAGE (csr5_sddmm.hip, csr5_refresh.hip): with T = 64 sigma, the entry of CSR rank e lies in tile t = e / T.  For
// t < p - 1 and raw tile_ptr[t] != tile_ptr[t + 1] (a moved tile) its column is stored at t T + ((e mod T) mod sigma) 64 +
// (e mod T) / sigma; fast-track tiles (raw words equal) and the CSR tail (t >= p - 1) are in CSR order.
//
// ROW CLASSES, decided per row on the device from L = row_ptr[i + 1] - row_ptr[i] and from nothing else; a workgroup of 256 lanes
// owns 256 consecutive rows, every wavefront 64 of them (lane l holds the bounds of row l):
//     L <= 16           16 lanes per row, 4 rows of the wavefront per pass.  Lane j computes s_j; maximum and Z by the 16-lane
//                       butterfly; then the 16 lanes own 16 output columns at a time and walk the row's entries.
//     17 <= L <= 512    one row at a time with all 64 lanes (ballot loop).  Scores and columns are staged in the wavefront's
//                       share of LDS (512 entries), overwritten by the weights; then lanes own output columns.
//     L > 512           listed in LDS and, after a barrier, worked on by the four wavefronts together.  Up to 2 048 entries are
//                       staged once (the four shares together); beyond that the maximum is taken in a first sweep that stores
//                       nothing and the scores are RECOMPUTED -- the same chain, the same bits -- chunk by chunk of 2 048 entries
//                       into the stage.  A lane holds the accumulators of 4 column blocks; d > 256 repeats the sweep per 256
//                       columns (and recomputes again beyond 2 048 entries).  One row is never split across workgroups.
//
// THE SUMMATION ORDER is a function of (L, d) alone.  j is an entry's rank inside its row.
//   Z, L <= 512:    slot(j) = j mod 64; every slot adds its w_j, j = slot, slot + 64, ..., in ascending order onto +0; the 64 slot
//                   sums (+0 for a slot without terms) by the balanced binary tree over adjacent slots (pairs, quads, ..., halves).
//                   L <= 16 runs the leading sub-tree over 16 slots: the same tree.  This is csr5hip_row_softmax's tree.
//   Z, L > 512:     slot(j) = j mod 256, slots 64 w .. 64 w + 63 by that tree (wavefront w), then (w0 + w1) + (w2 + w3).
//   acc_c, L <= 16: ONE chain acc = fma(w_j, V[j_j, c], acc) over j = 0 .. L-1 ascending onto +0.
//   acc_c, L > 16:  column c lies in block b = c / 64 of width wb = min(64, d - 64 b); C = the smallest power of two >= wb;
//                   S = 64 / C slots for L <= 512, S = 256 / C for L > 512.  slot(j) = j mod S; every slot runs ONE chain
//                   acc = fma(w_j, V[j_j, c], acc) over its j ascending onto +0; the S slot sums (+0 for a slot without terms)
//                   are added by the balanced binary tree over adjacent slots.
//
// DETERMINISM CONTRACT.  The bits of row i of O depend only on Q's row i, the K and V rows of the row's columns in their CSR
// order, k, d and the value type: not on sigma, any option, the kind of tile that holds the row's entries, the row's position,
// its neighbours, m, n, nnz, the leading dimensions, pointer alignment (16-byte and element loads feed the same chains) or the run.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

// the row classes' constants, the rank -> storage map and the score chain: shared with csr5_attention_bwd.hip
#include "csr5_attention_dev.h"

namespace csr5 {

template <typename VT>
struct AttArgs {
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

// ---- rows of at most 16 entries (empty rows included): 16 lanes per row, 4 rows of the wavefront per pass ------------------
template <typename VT, bool VEC>
__device__ __forceinline__ void att_short(const AttArgs<VT> &A, const long long row0, const int len, const int t0, const int rem0,
                                          const int h0, const int h1)
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
        int cj = 0; // the lane's column: loaded once, kept across the heads
        if (act)
            cj = A.col[att_storage(A, rt0, rrem, pos)];
        for (int h = h0; h < h1; h++) { // (uniform)
            const VT *Vh = A.V + (size_t)h * A.d;
            VT *Oh = A.O + (size_t)h * A.d;
            VT s = neg_inf<VT>();
            if (act)
                s = att_score<VT, VEC>(A.Q + r * A.ldq + (size_t)h * A.k, A.K + (size_t)(uint32_t)cj * A.ldk + (size_t)h * A.k, A.k);
            const VT mx = group_max<G>(s);
            const VT w = act ? exp_vt(s - mx) : (VT)0;
            const VT rinv = (VT)1 / group_sum<G>(w);
            for (int cb = 0; cb < A.d; cb += G) { // (uniform)
                const int c = cb + pos;
                VT acc = (VT)0;
                for (int e = 0; e < G; e++) {
                    if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                        break;
                    const VT we = __shfl(w, sub * G + e, OMEGA);
                    const int je = __shfl(cj, sub * G + e, OMEGA);
                    if (rowok && e < rl && c < A.d)
                        acc = fma_vt(we, Vh[(size_t)(uint32_t)je * A.ldv + c], acc);
                }
                if (rowok && c < A.d)
                    Oh[r * A.ldo + c] = rl > 0 ? acc * rinv : (VT)0;
            }
        }
    }
}

// ---- a row of 17 .. 512 entries: one wavefront; sc / cl: the wavefront's 512 staged scores (then weights) and columns ------
template <typename VT, bool VEC>
__device__ __forceinline__ void att_wave_row(const AttArgs<VT> &A, const size_t r, const int rl, const int t0, const int rem0, VT *sc,
                                             int *cl, const int h0, const int h1)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int h = h0; h < h1; h++) { // (uniform) cl is staged by the first head and kept; sc is refilled per head
        const VT *q = A.Q + r * A.ldq + (size_t)h * A.k;
        const VT *Kh = A.K + (size_t)h * A.k;
        VT mx = neg_inf<VT>();
        for (int j = lane; j < rl; j += OMEGA) { // (a lane reads back the columns it stored itself)
            int cj;
            if (h == h0) {
                cj = A.col[att_storage(A, t0, rem0, j)];
                cl[j] = cj;
            } else {
                cj = cl[j];
            }
            const VT s = att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k);
            sc[j] = s;
            mx = max_vt(mx, s);
        }
        mx = wave_max(mx);
        VT z = (VT)0;
        for (int j = lane; j < rl; j += OMEGA) { // (a lane reads back what it stored itself)
            const VT w = exp_vt(sc[j] - mx);
            sc[j] = w;
            z += w;
        }
        const VT rinv = (VT)1 / wave_sum(z);
        att_wave_sync();
        for (int cb = 0; cb < A.d; cb += OMEGA) {
            const int wb = A.d - cb < OMEGA ? A.d - cb : OMEGA;
            const int C = att_pow2(wb), S = OMEGA / C;
            const int slot = lane / C, cc = lane & (C - 1);
            VT acc = (VT)0;
            if (cc < wb) {
                const VT *v = A.V + (size_t)h * A.d + cb + cc;
#pragma unroll 4
                for (int e = slot; e < rl; e += S)
                    acc = fma_vt(sc[e], v[(size_t)(uint32_t)cl[e] * A.ldv], acc);
            }
            for (int off = C; off < OMEGA; off <<= 1) // (uniform; adjacent slots first)
                acc += __shfl_xor(acc, off, OMEGA);
            if (slot == 0 && cc < wb)
                A.O[r * A.ldo + (size_t)h * A.d + cb + cc] = acc * rinv;
        }
        att_wave_sync(); // (the next head's and the next row's scores stay behind these reads)
    }
}

// ---- a row beyond 512 entries: the workgroup; sc / cl: the AT_STAGE staged entries, red: AT_BLOCK values, red4: AT_WAVES -----
// One head of the row: q, Kh, Vh, o are that head's slices.  first: the head that stages cl of a row of at most AT_STAGE entries;
// the later heads take the columns from there.  (Beyond AT_STAGE entries the stage holds one chunk at a time and every head
// walks the pattern again: keeping the chunk across the heads would take 4 accumulators per head and lane.)
template <typename VT, bool VEC>
__device__ __forceinline__ void att_hub_head(const AttArgs<VT> &A, const VT *q, const VT *Kh, const VT *Vh, VT *o_row, const bool first,
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
        const VT s = att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k);
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
                    const int cj = A.col[att_storage(A, t0, rem0, base + jj)];
                    const VT w = exp_vt(att_score<VT, VEC>(q, Kh + (size_t)(uint32_t)cj * A.ldk, A.k) - mx);
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
                        const VT *v = Vh + cb + cc;
                        VT o = acc[b];
#pragma unroll 4
                        for (int e = slot; e < n; e += S)
                            o = fma_vt(sc[e], v[(size_t)(uint32_t)cl[e] * A.ldv], o);
                        acc[b] = o;
                    }
                }
            }
        }
        if (cg == 0)
            rinv = (VT)1 / block_combine<VT, false>(wave_sum(z), red4);
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
                    o_row[cb + tid] =
                        ((red[tid] + red[OMEGA + tid]) + (red[2 * OMEGA + tid] + red[3 * OMEGA + tid])) * rinv;
                __syncthreads(); // (red is free for the next block)
            }
        }
    }
    __syncthreads(); // (the stage is free for the next head or hub row)
}

template <typename VT, bool VEC>
__device__ __forceinline__ void att_hub_row(const AttArgs<VT> &A, const size_t r, const int rl, const int t0, const int rem0, VT *sc,
                                            int *cl, VT *red, VT *red4, const int h0, const int h1)
{
    for (int h = h0; h < h1; h++) // (uniform)
        att_hub_head<VT, VEC>(A, A.Q + r * A.ldq + (size_t)h * A.k, A.K + (size_t)h * A.k, A.V + (size_t)h * A.d,
                              A.O + r * A.ldo + (size_t)h * A.d, h == h0, rl, t0, rem0, sc, cl, red, red4);
}

// MH: the packed multi-head call (blockIdx.y owns a contiguous group of heads); otherwise exactly one head, known at compile time
template <typename VT, bool VEC, bool MH>
__global__ void __launch_bounds__(AT_BLOCK) k_attention(const AttArgs<VT> A)
{
    __shared__ VT sc[AT_STAGE];
    __shared__ int cl[AT_STAGE];
    __shared__ VT red[AT_BLOCK];
    __shared__ VT red4[AT_WAVES];
    __shared__ int hub_n;
    __shared__ int hub_row[AT_BLOCK];
    if (threadIdx.x == 0)
        hub_n = 0;
    __syncthreads();

    int h0 = 0, h1 = 1;
    if constexpr (MH) {
        h0 = (int)blockIdx.y * A.hper;
        h1 = A.heads - h0 < A.hper ? A.heads : h0 + A.hper;
    }
    const int wave = (int)(threadIdx.x >> 6);
    const long long row0 = (long long)blockIdx.x * AT_BLOCK + wave * OMEGA; // the wavefront's first row
    const long long r = (long long)blockIdx.x * AT_BLOCK + threadIdx.x;
    int a = 0, len = -1, t0 = 0, rem0 = 0;
    if (r < A.m) {
        a = A.row_ptr[r];
        len = A.row_ptr[r + 1] - a;
        len = len < 0 ? 0 : len;
        t0 = (int)((unsigned)a / (unsigned)A.T);
        rem0 = a - t0 * A.T;
    }
    att_short<VT, VEC>(A, row0, len, t0, rem0, h0, h1);

    unsigned long long todo = __ballot(len > AT_G && len <= AT_WAVE_ROW);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        att_wave_row<VT, VEC>(A, (size_t)(row0 + src), __builtin_amdgcn_readlane(len, src), __builtin_amdgcn_readlane(t0, src),
                              __builtin_amdgcn_readlane(rem0, src), sc + wave * AT_WAVE_ROW, cl + wave * AT_WAVE_ROW, h0, h1);
    }

    if (len > AT_WAVE_ROW)
        hub_row[atomicAdd(&hub_n, 1)] = (int)threadIdx.x; // (an integer counter in LDS: the order of the list decides no bit)
    __syncthreads(); // (and every wavefront is done with its share of the stage)
    const int hubs = __builtin_amdgcn_readfirstlane(hub_n);
    for (int i = 0; i < hubs; i++) { // (uniform over the workgroup: the barriers inside are reached by all)
        const long long hr = (long long)blockIdx.x * AT_BLOCK + __builtin_amdgcn_readfirstlane(hub_row[i]);
        const int ra = __builtin_amdgcn_readfirstlane(A.row_ptr[hr]);
        const int rl = __builtin_amdgcn_readfirstlane(A.row_ptr[hr + 1]) - ra;
        const int ht0 = (int)((unsigned)ra / (unsigned)A.T);
        att_hub_row<VT, VEC>(A, (size_t)hr, rl, ht0, ra - ht0 * A.T, sc, cl, red, red4, h0, h1);
    }
}

// heads == 1: the single-head instantiation.  groups: the head groups over grid.y, 0 for the rule (att_heads_per_group).
template <typename VT>
static hipError_t attention_typed(const Geometry &g, const DeviceArrays &d, int heads, int groups, const void *Q, int ldq, const void *K,
                                  int ldk, int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s)
{
    if (g.m <= 0 || dcols <= 0 || heads <= 0)
        return hipSuccess;
    AttArgs<VT> A;
    A.m = g.m;
    A.k = k;
    A.d = dcols;
    A.heads = heads;
    A.hper = groups > 0 ? (heads + groups - 1) / groups : att_heads_per_group(g.m, heads);
    A.sigma = g.sigma > 0 ? g.sigma : 1;
    A.T = g.tile_elems > 0 ? g.tile_elems : OMEGA;
    A.tiles = g.p > 1 ? g.p - 1 : 0;
    A.recip = (1u << 20) / (unsigned)A.sigma + 1u;
    A.row_ptr = d.row_ptr;
    A.col = d.col;
    A.tile_ptr = d.tile_ptr;
    A.Q = (const VT *)Q;
    A.K = (const VT *)K;
    A.V = (const VT *)V;
    A.O = (VT *)O;
    A.ldq = ldq;
    A.ldk = ldk;
    A.ldv = ldv;
    A.ldo = ldo;
    // 16-byte loads: at least one whole block, and every head's slice of every row of Q and of K starts on a 16-byte boundary
    const bool vec = k >= 32 / (int)sizeof(VT) && reinterpret_cast<uintptr_t>(Q) % 16 == 0 && reinterpret_cast<uintptr_t>(K) % 16 == 0 &&
                     ((size_t)ldq * sizeof(VT)) % 16 == 0 && ((size_t)ldk * sizeof(VT)) % 16 == 0 &&
                     (heads == 1 || ((size_t)k * sizeof(VT)) % 16 == 0);
    const unsigned blocks = (unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK);
    const dim3 block(AT_BLOCK);
    if (heads == 1) {
        const dim3 grid(blocks);
        if (vec)
            hipLaunchKernelGGL((k_attention<VT, true, false>), grid, block, 0, s, A);
        else
            hipLaunchKernelGGL((k_attention<VT, false, false>), grid, block, 0, s, A);
    } else {
        const dim3 grid(blocks, (unsigned)((heads + A.hper - 1) / A.hper));
        if (vec)
            hipLaunchKernelGGL((k_attention<VT, true, true>), grid, block, 0, s, A);
        else
            hipLaunchKernelGGL((k_attention<VT, false, true>), grid, block, 0, s, A);
    }
    return hipGetLastError();
}

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / -DCSR5_ATTENTION_ONLY_F32), as csr5_sddmm.hip.
#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_f64(const Geometry &g, const DeviceArrays &d, int heads, int groups, const void *Q, int ldq, const void *K, int ldk,
                          int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s)
{
    return attention_typed<double>(g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s);
}
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
hipError_t launch_mha_f32(const Geometry &g, const DeviceArrays &d, int heads, int groups, const void *Q, int ldq, const void *K, int ldk,
                          int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s)
{
    return attention_typed<float>(g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s);
}
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_mha_f32(const Geometry &g, const DeviceArrays &d, int heads, int groups, const void *Q, int ldq, const void *K, int ldk,
                          int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s);

hipError_t launch_mha(const Geometry &g, const DeviceArrays &d, int value_type, int heads, int groups, const void *Q, int ldq,
                      const void *K, int ldk, int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_mha_f64(g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s)
                                     : launch_mha_f32(g, d, heads, groups, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s);
}

hipError_t launch_attention(const Geometry &g, const DeviceArrays &d, int value_type, const void *Q, int ldq, const void *K, int ldk,
                            int k, const void *V, int ldv, int dcols, void *O, int ldo, hipStream_t s)
{
    return launch_mha(g, d, value_type, 1, 0, Q, ldq, K, ldk, k, V, ldv, dcols, O, ldo, s);
}
#endif

} // namespace csr5
