// csr5_reduce_kern.h -- the kernel templates of csr5hip_spmm_reduce and csr5hip_spmm_reduce_backward and their typed launchers; the
// contract is include/csr5hip_reduce.h.  One translation unit instantiates them (csr5_reduce.hip); the host emulation compiles them
// as plain C++ (scripts/host_emulation/reduce_driver.cpp).
// The three kernels walk rows by row_ptr with the attention kernels' row classes (csr5_attention_kern.h): 16 lanes for a row of at
// most AT_G entries, a wavefront up to AT_WAVE_ROW, the workgroup beyond, in chunks of AT_STAGE; an entry's column and value are read
// through att_storage.  Nothing of the CSR5 segmented sum is used: a maximum has no carries.
//   k_spmm_reduce       the forward.  Where attention runs its product stage this kernel runs the same lane layout -- lanes along the
//                       output columns (C = att_pow2(width)), 64 / C or 256 / C entry slots, columns in blocks of 64 -- with the fma
//                       accumulator replaced by a (value, rank) pair under the contract's order (red_beats).  The order is total,
//                       so the winner does not depend on how entries are dealt to slots or in which order slots are combined.
//   k_spmm_reduce_dval  a row kernel, one entry per lane slot: the entry's chain over the c where arg[i, c] is its own rank.
//   k_spmm_reduce_dx    the column kernel on the transposed companion, lanes along c, the summation tree of the contract.
// Include it after `#pragma clang fp contract(off)`; gfx950 (wave64) only.
#pragma once

#include "csr5_attention_dev.h"

namespace csr5 {

constexpr int RED_NONE = 0x7FFFFFFF; // the rank of "no entry yet": it loses every tie, and its value (red_start) every comparison

// the pattern walked (att_storage reads T, sigma, tiles, recip and tile_ptr) and the operands of the forward
template <typename VT>
struct RedArgs {
    int m, k;
    int T, sigma, tiles;
    unsigned recip;
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const VT *val; // the handle's values in tile order; read only when WEIGHTED
    const VT *X;
    VT *Y;
    int32_t *arg;  // written only when ARG
    int ldx, ldy, ldarg;
};

// the backward's: dval walks the parent's pattern (map and val unused, out = dval), dx the companion's (X unused, out = dX)
template <typename VT>
struct RedBwdArgs {
    int m, k; // m: the lines of the pattern walked
    int T, sigma, tiles;
    unsigned recip;
    const int32_t *row_ptr;
    const int32_t *col;
    const uint32_t *tile_ptr;
    const VT *val;       // dx, WEIGHTED: the companion's copy of the values, in its tile order
    const uint32_t *map; // dx: position in A^T's CSR -> rank in A's CSR
    const VT *X;
    const VT *dY;
    const int32_t *arg;
    VT *out;
    int ldx, lddy, ldarg, ldo;
};

// whether (va, ra) beats (vb, rb): the contract's order.  NaN first, then the larger (MAX) or smaller (MIN) value, then the smaller rank
template <int OP, typename VT>
__device__ __forceinline__ bool red_beats(const VT va, const int ra, const VT vb, const int rb)
{
    const bool na = va != va, nb = vb != vb;
    if (na != nb)
        return na;
    if (!na && va != vb)
        return OP == CSR5HIP_REDUCE_MAX ? va > vb : va < vb;
    return ra < rb;
}
template <int OP, typename VT>
__device__ __forceinline__ void red_take(VT &v, int &r, const VT ov, const int orr)
{
    if (red_beats<OP>(ov, orr, v, r)) {
        v = ov;
        r = orr;
    }
}
// the value that goes with RED_NONE: -Inf (MAX) / +Inf (MIN) loses to every number, to NaN, and by rank to an entry that equals it
template <int OP, typename VT>
__device__ __forceinline__ VT red_start()
{
    return OP == CSR5HIP_REDUCE_MAX ? neg_inf<VT>() : -neg_inf<VT>();
}

// ---- forward: rows of at most 16 entries (empty rows included): 16 lanes per row, 4 rows of the wavefront per pass; a lane keeps
// its entry's column (and value) and hands it round by shuffles, as att_short does ------------------------------------------------
template <typename VT, int OP, bool WEIGHTED, bool ARG>
__device__ __forceinline__ void red_short(const RedArgs<VT> &A, const long long row0, const int len, const int a, const int t0,
                                          const int rem0)
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
        const int ra = __shfl(a, src, OMEGA);
        const int rt0 = __shfl(t0, src, OMEGA);
        const int rrem = __shfl(rem0, src, OMEGA);
        const bool rowok = (cls >> src) & 1;
        const bool act = rowok && pos < rl;
        const size_t r = (size_t)(row0 + src);
        int cj = 0;
        VT av = (VT)0;
        if (act) {
            const size_t st = att_storage(A, rt0, rrem, pos);
            cj = A.col[st];
            if constexpr (WEIGHTED)
                av = A.val[st];
        }
        for (int cb = 0; cb < A.k; cb += G) { // (uniform)
            const int c = cb + pos;
            VT bv = red_start<OP, VT>();
            int br = RED_NONE;
            for (int e = 0; e < G; e++) {
                if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                    break;
                const int je = __shfl(cj, sub * G + e, OMEGA);
                VT ae = (VT)0;
                if constexpr (WEIGHTED)
                    ae = __shfl(av, sub * G + e, OMEGA);
                if (rowok && e < rl && c < A.k) {
                    const VT x = A.X[(size_t)(uint32_t)je * A.ldx + c];
                    VT t = x;
                    if constexpr (WEIGHTED)
                        t = ae * x;
                    red_take<OP>(bv, br, t, ra + e);
                }
            }
            if (rowok && c < A.k) {
                A.Y[r * A.ldy + c] = rl > 0 ? bv : (VT)0;
                if constexpr (ARG)
                    A.arg[r * A.ldarg + c] = rl > 0 ? br : -1;
            }
        }
    }
}

// ---- forward: a row of 17 .. 512 entries: one wavefront; cl / sc: the wavefront's staged columns and (WEIGHTED) values --------------
template <typename VT, int OP, bool WEIGHTED, bool ARG>
__device__ __forceinline__ void red_wave_row(const RedArgs<VT> &A, const size_t r, const int rl, const int ra, const int t0,
                                             const int rem0, VT *sc, int *cl)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int j = lane; j < rl; j += OMEGA) {
        const size_t st = att_storage(A, t0, rem0, j);
        cl[j] = A.col[st];
        if constexpr (WEIGHTED)
            sc[j] = A.val[st];
    }
    att_wave_sync();
    for (int cb = 0; cb < A.k; cb += OMEGA) { // (uniform)
        const int wb = A.k - cb < OMEGA ? A.k - cb : OMEGA;
        const int C = att_pow2(wb), S = OMEGA / C;
        const int slot = lane / C, cc = lane & (C - 1);
        VT bv = red_start<OP, VT>();
        int br = RED_NONE;
        if (cc < wb) {
            const VT *x = A.X + cb + cc;
#pragma unroll 4
            for (int e = slot; e < rl; e += S) {
                VT t = x[(size_t)(uint32_t)cl[e] * A.ldx];
                if constexpr (WEIGHTED)
                    t = sc[e] * t;
                red_take<OP>(bv, br, t, ra + e);
            }
        }
        for (int off = C; off < OMEGA; off <<= 1) { // (uniform) the slots' pairs under the same order
            const VT ov = __shfl_xor(bv, off, OMEGA);
            const int orr = __shfl_xor(br, off, OMEGA);
            red_take<OP>(bv, br, ov, orr);
        }
        if (slot == 0 && cc < wb) {
            A.Y[r * A.ldy + cb + cc] = bv;
            if constexpr (ARG)
                A.arg[r * A.ldarg + cb + cc] = br;
        }
    }
    att_wave_sync(); // (the next row's stage stays behind these reads)
}

// ---- forward: a row beyond 512 entries: the workgroup, chunk by chunk of AT_STAGE entries, the pairs of AT_HUB_BLOCKS column blocks
// kept in registers across the chunks; redv / redr: AT_BLOCK pairs, the four wavefronts' results of one column block ---------------
template <typename VT, int OP, bool WEIGHTED, bool ARG>
__device__ __forceinline__ void red_hub_row(const RedArgs<VT> &A, const size_t r, const int rl, const int ra, const int t0,
                                            const int rem0, VT *sc, int *cl, VT *redv, int *redr)
{
    const int tid = (int)threadIdx.x;
    for (int cg = 0; cg < A.k; cg += OMEGA * AT_HUB_BLOCKS) { // (uniform over the workgroup, as every loop bound and barrier below)
        VT bv[AT_HUB_BLOCKS];
        int br[AT_HUB_BLOCKS];
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            bv[b] = red_start<OP, VT>();
            br[b] = RED_NONE;
        }
        for (int base = 0; base < rl; base += AT_STAGE) {
            const int n = rl - base < AT_STAGE ? rl - base : AT_STAGE;
            __syncthreads(); // (the stage is free: the previous chunk has been read)
            for (int jj = tid; jj < n; jj += AT_BLOCK) {
                const size_t st = att_storage(A, t0, rem0, base + jj);
                cl[jj] = A.col[st];
                if constexpr (WEIGHTED)
                    sc[jj] = A.val[st];
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < AT_HUB_BLOCKS; b++) {
                const int cb = cg + b * OMEGA;
                if (cb < A.k) {
                    const int wb = A.k - cb < OMEGA ? A.k - cb : OMEGA;
                    const int C = att_pow2(wb), S = AT_BLOCK / C;
                    const int slot = tid / C, cc = tid & (C - 1);
                    if (cc < wb) {
                        const VT *x = A.X + cb + cc;
                        VT v = bv[b];
                        int rr = br[b];
#pragma unroll 4
                        for (int e = slot; e < n; e += S) {
                            VT t = x[(size_t)(uint32_t)cl[e] * A.ldx];
                            if constexpr (WEIGHTED)
                                t = sc[e] * t;
                            red_take<OP>(v, rr, t, ra + base + e);
                        }
                        bv[b] = v;
                        br[b] = rr;
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < AT_HUB_BLOCKS; b++) {
            const int cb = cg + b * OMEGA;
            if (cb < A.k) { // (uniform)
                const int wb = A.k - cb < OMEGA ? A.k - cb : OMEGA;
                const int C = att_pow2(wb);
                VT v = bv[b];
                int rr = br[b];
                for (int off = C; off < OMEGA; off <<= 1) { // the slots of the wavefront ...
                    const VT ov = __shfl_xor(v, off, OMEGA);
                    const int orr = __shfl_xor(rr, off, OMEGA);
                    red_take<OP>(v, rr, ov, orr);
                }
                redv[tid] = v;
                redr[tid] = rr;
                __syncthreads();
                if (tid < wb) { // ... then the four wavefronts; lane c < C of every wavefront holds column c
                    v = redv[tid];
                    rr = redr[tid];
                    red_take<OP>(v, rr, redv[OMEGA + tid], redr[OMEGA + tid]);
                    red_take<OP>(v, rr, redv[2 * OMEGA + tid], redr[2 * OMEGA + tid]);
                    red_take<OP>(v, rr, redv[3 * OMEGA + tid], redr[3 * OMEGA + tid]);
                    A.Y[r * A.ldy + cb + tid] = v;
                    if constexpr (ARG)
                        A.arg[r * A.ldarg + cb + tid] = rr;
                }
                __syncthreads(); // (redv / redr are free for the next block)
            }
        }
    }
    __syncthreads(); // (the stage is free for the next hub row)
}

// The skeleton of CSR5_ATTENTION_KERNEL_BODY, shared by the three kernels: each lane reads one row's bounds; then SHORT, the ballot
// loop over the wavefront's rows (WAVE) and the LDS list of the workgroup's hub rows (HUB).  A MACRO for that macro's reason.  In
// scope for the three statements: A, wave, row0; SHORT: len, a, t0, rem0 (per lane); WAVE and HUB: wr (the row), wl, wa, wt0, wrem
// (uniform)
#define CSR5_REDUCE_KERNEL_BODY(SHORT, WAVE, HUB)                                                                                  \
    __shared__ int hub_n;                                                                                                          \
    __shared__ int hub_row[AT_BLOCK];                                                                                              \
    if (threadIdx.x == 0)                                                                                                          \
        hub_n = 0;                                                                                                                 \
    __syncthreads();                                                                                                               \
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
    SHORT;                                                                                                                         \
    unsigned long long todo = __ballot(len > AT_G && len <= AT_WAVE_ROW);                                                          \
    while (todo) {                                                                                                                 \
        const int src = __builtin_ctzll(todo);                                                                                     \
        todo &= todo - 1;                                                                                                          \
        const size_t wr = (size_t)(row0 + src);                                                                                    \
        const int wl = __builtin_amdgcn_readlane(len, src), wa = __builtin_amdgcn_readlane(a, src);                                \
        const int wt0 = __builtin_amdgcn_readlane(t0, src), wrem = __builtin_amdgcn_readlane(rem0, src);                           \
        WAVE;                                                                                                                      \
    }                                                                                                                              \
    if (len > AT_WAVE_ROW)                                                                                                         \
        hub_row[atomicAdd(&hub_n, 1)] = (int)threadIdx.x; /* (an integer counter in LDS: the order of the list decides no bit) */  \
    __syncthreads(); /* (and every wavefront is done with its share of the stage) */                                               \
    const int hubs = __builtin_amdgcn_readfirstlane(hub_n);                                                                        \
    for (int i = 0; i < hubs; i++) { /* (uniform over the workgroup: the barriers inside are reached by all) */                    \
        const size_t wr = (size_t)((long long)blockIdx.x * AT_BLOCK + __builtin_amdgcn_readfirstlane(hub_row[i]));                 \
        const int wa = __builtin_amdgcn_readfirstlane(A.row_ptr[wr]);                                                              \
        const int wl = __builtin_amdgcn_readfirstlane(A.row_ptr[wr + 1]) - wa;                                                     \
        const int wt0 = (int)((unsigned)wa / (unsigned)A.T), wrem = wa - wt0 * A.T;                                                \
        HUB;                                                                                                                       \
    }

template <typename VT, int OP, bool WEIGHTED, bool ARG>
__global__ void __launch_bounds__(AT_BLOCK) k_spmm_reduce(const RedArgs<VT> A)
{
    __shared__ VT sc[AT_STAGE];
    __shared__ int cl[AT_STAGE];
    __shared__ VT redv[AT_BLOCK];
    __shared__ int redr[AT_BLOCK];
    CSR5_REDUCE_KERNEL_BODY((red_short<VT, OP, WEIGHTED, ARG>(A, row0, len, a, t0, rem0)),
                            (red_wave_row<VT, OP, WEIGHTED, ARG>(A, wr, wl, wa, wt0, wrem, sc + wave * AT_WAVE_ROW, cl + wave * AT_WAVE_ROW)),
                            (red_hub_row<VT, OP, WEIGHTED, ARG>(A, wr, wl, wa, wt0, wrem, sc, cl, redv, redr)))
}

// ---- dval: the chain of entry e = (i, cj): acc = fma(X[cj, c], dY[i, c], acc) from +0 over the c with arg[i, c] == e, ascending.  The
// rows of arg and of dY are the same addresses for all lanes of a row; arg is compared, never used as an index ----------------------
template <typename VT>
__device__ __forceinline__ VT red_dval_chain(const RedBwdArgs<VT> &A, const size_t i, const int e, const int cj)
{
    const int32_t *ar = A.arg + i * A.ldarg;
    const VT *g = A.dY + i * A.lddy;
    const VT *x = A.X + (size_t)(uint32_t)cj * A.ldx;
    VT acc = (VT)0;
#pragma unroll 4
    for (int c = 0; c < A.k; c++)
        if (ar[c] == e)
            acc = fma_vt(x[c], g[c], acc);
    return acc;
}

template <typename VT>
__device__ __forceinline__ void red_dval_short(const RedBwdArgs<VT> &A, const long long row0, const int len, const int a, const int t0,
                                               const int rem0)
{
    constexpr int G = AT_G, ROWS = OMEGA / G;
    const int lane = threadIdx.x & (OMEGA - 1);
    const int sub = lane / G, pos = lane % G;
    const unsigned long long cls = __ballot(len > 0 && len <= G);
    if (!cls)
        return;
    for (int pass = 0; pass < G; pass++) {
        const unsigned long long here = (cls >> (pass * ROWS)) & ((1ull << ROWS) - 1);
        if (!here) // (wave-uniform)
            continue;
        const int src = pass * ROWS + sub;
        const int rl = __shfl(len, src, OMEGA);
        const int ra = __shfl(a, src, OMEGA);
        const int rt0 = __shfl(t0, src, OMEGA);
        const int rrem = __shfl(rem0, src, OMEGA);
        if (((cls >> src) & 1) && pos < rl)
            A.out[(size_t)ra + pos] = red_dval_chain(A, (size_t)(row0 + src), ra + pos, A.col[att_storage(A, rt0, rrem, pos)]);
    }
}

// a row of more than 16 entries: its entries dealt to `lanes` lanes from `first` on
template <typename VT>
__device__ __forceinline__ void red_dval_row(const RedBwdArgs<VT> &A, const size_t r, const int rl, const int ra, const int t0,
                                             const int rem0, const int first, const int lanes)
{
    for (int j = first; j < rl; j += lanes)
        A.out[(size_t)ra + j] = red_dval_chain(A, r, ra + j, A.col[att_storage(A, t0, rem0, j)]);
}

template <typename VT>
__global__ void __launch_bounds__(AT_BLOCK) k_spmm_reduce_dval(const RedBwdArgs<VT> A)
{
    CSR5_REDUCE_KERNEL_BODY((red_dval_short<VT>(A, row0, len, a, t0, rem0)),
                            (red_dval_row<VT>(A, wr, wl, wa, wt0, wrem, (int)(threadIdx.x & (OMEGA - 1)), OMEGA)),
                            (red_dval_row<VT>(A, wr, wl, wa, wt0, wrem, (int)threadIdx.x, AT_BLOCK)))
}

// ---- dx: a line j of the companion is column j of A; position p of the line is the entry of A with rank map[row_ptr[j] + p], in
// A's row col[storage], with the value val[storage].  Its term in column c: the product where arg names it, +0 where not ---------
template <typename VT, bool WEIGHTED>
__device__ __forceinline__ VT red_dx_term(const RedBwdArgs<VT> &A, const int i, const int e, const VT av, const int c)
{
    if (A.arg[(size_t)(uint32_t)i * A.ldarg + c] != e)
        return (VT)0;
    const VT g = A.dY[(size_t)(uint32_t)i * A.lddy + c];
    if constexpr (WEIGHTED)
        return av * g;
    else
        return g;
}

// lines of at most 16 entries: ONE chain in ascending position; 16 lanes per line along c, the entries handed round by shuffles
template <typename VT, bool WEIGHTED>
__device__ __forceinline__ void red_dx_short(const RedBwdArgs<VT> &A, const long long row0, const int len, const int a, const int t0,
                                             const int rem0)
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
        const int ra = __shfl(a, src, OMEGA);
        const int rt0 = __shfl(t0, src, OMEGA);
        const int rrem = __shfl(rem0, src, OMEGA);
        const bool rowok = (cls >> src) & 1;
        const size_t j = (size_t)(row0 + src);
        int ei = 0, ee = -1;
        VT av = (VT)0;
        if (rowok && pos < rl) {
            const size_t st = att_storage(A, rt0, rrem, pos);
            ei = A.col[st];
            ee = (int)A.map[(size_t)ra + pos];
            if constexpr (WEIGHTED)
                av = A.val[st];
        }
        for (int cb = 0; cb < A.k; cb += G) { // (uniform)
            const int c = cb + pos;
            VT acc = (VT)0;
            for (int e = 0; e < G; e++) {
                if (!__any(rowok && e < rl)) // (uniform: the shuffles below are executed by every lane)
                    break;
                const int ie = __shfl(ei, sub * G + e, OMEGA);
                const int re = __shfl(ee, sub * G + e, OMEGA);
                VT ae = (VT)0;
                if constexpr (WEIGHTED)
                    ae = __shfl(av, sub * G + e, OMEGA);
                if (rowok && e < rl && c < A.k)
                    acc = acc + red_dx_term<VT, WEIGHTED>(A, ie, re, ae, c);
            }
            if (rowok && c < A.k)
                A.out[j * A.ldo + c] = acc;
        }
    }
}

// One wavefront's four chains of a line, over the positions first + q + n stride (q = 0 .. 3 the chain, n = 0, 1, ...), for the column
// block of wb columns at cb: (c0 + c1) + (c2 + c3), valid in the lanes below wb.  SL = min(64 / C, 4) entry slots hold 4 / SL chains
// each: slot s the chains s, s + SL, ...; the slots are added first, then a lane's registers -- the same tree whatever C is.
template <typename VT, bool WEIGHTED>
__device__ __forceinline__ VT red_dx_chains(const RedBwdArgs<VT> &A, const int rl, const int ra, const int t0, const int rem0,
                                            const int first, const int stride, const int cb, const int wb)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    const int C = att_pow2(wb);
    const int SL = OMEGA / C < 4 ? OMEGA / C : 4, NR = 4 / SL;
    const int slot = lane / C, cc = lane & (C - 1);
    const bool active = slot < SL && cc < wb;
    VT acc[4] = {(VT)0, (VT)0, (VT)0, (VT)0};
    for (int p0 = first; p0 < rl; p0 += stride) { // (uniform)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int p = p0 + slot + i * SL;
            if (i < NR && active && p < rl) {
                const size_t st = att_storage(A, t0, rem0, p);
                VT av = (VT)0;
                if constexpr (WEIGHTED)
                    av = A.val[st];
                acc[i] = acc[i] + red_dx_term<VT, WEIGHTED>(A, A.col[st], (int)A.map[(size_t)ra + p], av, cb + cc);
            }
        }
    }
    for (int off = C; off < C * SL; off <<= 1) { // (uniform) adjacent slots first
#pragma unroll
        for (int i = 0; i < 4; i++)
            acc[i] += __shfl_xor(acc[i], off, OMEGA);
    }
    return NR == 4 ? (acc[0] + acc[1]) + (acc[2] + acc[3]) : NR == 2 ? acc[0] + acc[1] : acc[0];
}

// a line of 17 .. 512 entries: one wavefront, four chains by position mod 4
template <typename VT, bool WEIGHTED>
__device__ __forceinline__ void red_dx_wave_row(const RedBwdArgs<VT> &A, const size_t j, const int rl, const int ra, const int t0,
                                                const int rem0)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    for (int cb = 0; cb < A.k; cb += OMEGA) { // (uniform)
        const int wb = A.k - cb < OMEGA ? A.k - cb : OMEGA;
        const VT v = red_dx_chains<VT, WEIGHTED>(A, rl, ra, t0, rem0, 0, 4, cb, wb);
        if (lane < wb)
            A.out[j * A.ldo + cb + lane] = v;
    }
}

// a line beyond 512 entries: the workgroup, sixteen chains by position mod 16, wavefront w the chains 4 w .. 4 w + 3; red: AT_BLOCK values
template <typename VT, bool WEIGHTED>
__device__ __forceinline__ void red_dx_hub_row(const RedBwdArgs<VT> &A, const size_t j, const int rl, const int ra, const int t0,
                                               const int rem0, VT *red)
{
    const int tid = (int)threadIdx.x;
    for (int cb = 0; cb < A.k; cb += OMEGA) { // (uniform over the workgroup)
        const int wb = A.k - cb < OMEGA ? A.k - cb : OMEGA;
        red[tid] = red_dx_chains<VT, WEIGHTED>(A, rl, ra, t0, rem0, 4 * (tid >> 6), 16, cb, wb);
        __syncthreads();
        if (tid < wb)
            A.out[j * A.ldo + cb + tid] = (red[tid] + red[OMEGA + tid]) + (red[2 * OMEGA + tid] + red[3 * OMEGA + tid]);
        __syncthreads(); // (red is free for the next block)
    }
}

template <typename VT, bool WEIGHTED>
__global__ void __launch_bounds__(AT_BLOCK) k_spmm_reduce_dx(const RedBwdArgs<VT> A)
{
    __shared__ VT red[AT_BLOCK];
    CSR5_REDUCE_KERNEL_BODY((red_dx_short<VT, WEIGHTED>(A, row0, len, a, t0, rem0)),
                            (red_dx_wave_row<VT, WEIGHTED>(A, wr, wl, wa, wt0, wrem)),
                            (red_dx_hub_row<VT, WEIGHTED>(A, wr, wl, wa, wt0, wrem, red)))
}

// ---- the typed launchers ---------------------------------------------------------------------------------------------------------
template <typename ARGS>
static void reduce_fill_pattern(ARGS &A, const Geometry &g, const DeviceArrays &d, const int k)
{
    A.m = g.m;
    A.k = k;
    A.sigma = g.sigma > 0 ? g.sigma : 1;
    A.T = g.tile_elems > 0 ? g.tile_elems : OMEGA;
    A.tiles = g.p > 1 ? g.p - 1 : 0;
    A.recip = (1u << 20) / (unsigned)A.sigma + 1u;
    A.row_ptr = d.row_ptr;
    A.col = d.col;
    A.tile_ptr = d.tile_ptr;
}

template <typename VT, int OP, bool WEIGHTED>
static void reduce_enqueue(const RedArgs<VT> &A, const dim3 grid, hipStream_t s)
{
    if (A.arg)
        hipLaunchKernelGGL((k_spmm_reduce<VT, OP, WEIGHTED, true>), grid, dim3(AT_BLOCK), 0, s, A);
    else
        hipLaunchKernelGGL((k_spmm_reduce<VT, OP, WEIGHTED, false>), grid, dim3(AT_BLOCK), 0, s, A);
}

template <typename VT>
static hipError_t reduce_typed(const Geometry &g, const DeviceArrays &d, int op, int weighted, const void *X, int ldx, int k, void *Y,
                               int ldy, int32_t *arg, int ldarg, hipStream_t s)
{
    if (g.m <= 0 || k <= 0)
        return hipSuccess;
    RedArgs<VT> A;
    reduce_fill_pattern(A, g, d, k);
    A.val = weighted ? (const VT *)d.val : nullptr;
    A.X = (const VT *)X;
    A.Y = (VT *)Y;
    A.arg = arg;
    A.ldx = ldx;
    A.ldy = ldy;
    A.ldarg = ldarg;
    const dim3 grid((unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK));
    if (op == CSR5HIP_REDUCE_MAX) {
        if (weighted)
            reduce_enqueue<VT, CSR5HIP_REDUCE_MAX, true>(A, grid, s);
        else
            reduce_enqueue<VT, CSR5HIP_REDUCE_MAX, false>(A, grid, s);
    } else {
        if (weighted)
            reduce_enqueue<VT, CSR5HIP_REDUCE_MIN, true>(A, grid, s);
        else
            reduce_enqueue<VT, CSR5HIP_REDUCE_MIN, false>(A, grid, s);
    }
    return hipGetLastError();
}

template <typename VT>
static hipError_t reduce_dval_typed(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, const void *dY, int lddy,
                                    const int32_t *arg, int ldarg, void *dval, hipStream_t s)
{
    if (g.m <= 0 || g.nnz <= 0)
        return hipSuccess;
    RedBwdArgs<VT> A;
    reduce_fill_pattern(A, g, d, k);
    A.val = nullptr;
    A.map = nullptr;
    A.X = (const VT *)X;
    A.dY = (const VT *)dY;
    A.arg = arg;
    A.out = (VT *)dval;
    A.ldx = ldx;
    A.lddy = lddy;
    A.ldarg = ldarg;
    A.ldo = 0;
    const dim3 grid((unsigned)(((long long)g.m + AT_BLOCK - 1) / AT_BLOCK));
    hipLaunchKernelGGL((k_spmm_reduce_dval<VT>), grid, dim3(AT_BLOCK), 0, s, A);
    return hipGetLastError();
}

template <typename VT>
static hipError_t reduce_dx_typed(const Geometry &gt, const DeviceArrays &dt, const uint32_t *map, int weighted, int k, const void *dY,
                                  int lddy, const int32_t *arg, int ldarg, void *dX, int lddx, hipStream_t s)
{
    if (gt.m <= 0 || k <= 0)
        return hipSuccess;
    RedBwdArgs<VT> A;
    reduce_fill_pattern(A, gt, dt, k);
    A.val = weighted ? (const VT *)dt.val : nullptr;
    A.map = map;
    A.X = nullptr;
    A.dY = (const VT *)dY;
    A.arg = arg;
    A.out = (VT *)dX;
    A.ldx = 0;
    A.lddy = lddy;
    A.ldarg = ldarg;
    A.ldo = lddx;
    const dim3 grid((unsigned)(((long long)gt.m + AT_BLOCK - 1) / AT_BLOCK));
    if (weighted)
        hipLaunchKernelGGL((k_spmm_reduce_dx<VT, true>), grid, dim3(AT_BLOCK), 0, s, A);
    else
        hipLaunchKernelGGL((k_spmm_reduce_dx<VT, false>), grid, dim3(AT_BLOCK), 0, s, A);
    return hipGetLastError();
}

} // namespace csr5
