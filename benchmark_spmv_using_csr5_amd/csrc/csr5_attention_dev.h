// csr5_attention_dev.h -- the device helpers that csr5_attention.hip (forward) and csr5_attention_bwd.hip (backward) share, so
// that both take an entry's column by ONE rank -> storage rule and compute a score by ONE chain: the backward recomputes the
// forward's scores and must get the same bits.  Include it after `#pragma clang fp contract(off)`; gfx950 (wave64) only.
#pragma once

#include "csr5_internal.h"
#include "csr5_wave.h"

namespace csr5 {

constexpr int AT_BLOCK = 256;                      // lanes = rows of a workgroup
constexpr int AT_WAVES = AT_BLOCK / OMEGA;
constexpr int AT_G = 16;                           // lanes of a short row; rows up to this many entries are short
constexpr int AT_WAVE_ROW = 512;                   // entries a wavefront stages: rows up to this length are one wavefront's
constexpr int AT_STAGE = AT_WAVES * AT_WAVE_ROW;   // entries the workgroup stages: a hub row's chunk
constexpr int AT_HUB_BLOCKS = 4;                   // column blocks of 64 whose accumulators a lane of a hub row holds

// Heads of one workgroup of a packed multi-head launch; grid.y = ceil(heads / this) contiguous head groups.  A function of the
// pattern's line count and of heads, of nothing else: enough groups to bring the grid to AT_GRID_TARGET workgroups (256 compute
// units, 4 workgroups each), but at most ceil(heads / 2) groups, so that the pattern work is shared wherever two heads are left
// to share it (an odd head count leaves the last group of a two-head split with one head).  No bit depends on it.
constexpr long long AT_GRID_TARGET = 1024;
inline int att_heads_per_group(const long long lines, const int heads)
{
    const long long blocks = lines > 0 ? (lines + AT_BLOCK - 1) / AT_BLOCK : 1;
    long long groups = (AT_GRID_TARGET + blocks - 1) / blocks;
    const long long cap = ((long long)heads + 1) / 2;
    groups = groups < cap ? groups : cap;
    groups = groups < 1 ? 1 : groups;
    return (int)((heads + groups - 1) / groups);
}

// storage position of the entry of rank j inside a row whose first entry has CSR rank t0 * T + rem0.  ARGS carries the pattern:
// T (tile_elems), sigma, tiles (p - 1), recip (sigma's reciprocal in 20 fractional bits, rounded up) and tile_ptr.
template <typename ARGS>
__device__ __forceinline__ size_t att_storage(const ARGS &A, const int t0, const int rem0, const int j)
{
    unsigned x = (unsigned)rem0 + (unsigned)j;
    int t = t0;
    if (x >= (unsigned)A.T) {
        const unsigned q = x / (unsigned)A.T;
        t += (int)q;
        x -= q * (unsigned)A.T;
    }
    const size_t base = (size_t)t * A.T;
    if (t >= A.tiles || A.tile_ptr[t] == A.tile_ptr[t + 1])
        return base + x; // CSR tail / fast-track tile: CSR order
    const unsigned l = (x * A.recip) >> 20; // x / sigma: exact for x < 2 048, sigma <= 32
    const unsigned i = x - l * (unsigned)A.sigma;
    return base + (size_t)i * OMEGA + l;
}

// 16 bytes of a row of the storage type ST, converted to the compute type VT.  ST == VT: the words as they are; a 2-byte ST (bf16,
// fp16; csr5_attention_lowp.hip): 8 elements, each widened exactly by the cast.
template <typename ST, typename VT>
__device__ __forceinline__ void att_load16(const ST *__restrict__ p, VT *o)
{
    const uint4 w = *reinterpret_cast<const uint4 *>(p);
    if constexpr (sizeof(ST) == 8) {
        o[0] = __builtin_bit_cast(double, (unsigned long long)w.y << 32 | w.x);
        o[1] = __builtin_bit_cast(double, (unsigned long long)w.w << 32 | w.z);
    } else if constexpr (sizeof(ST) == 4) {
        o[0] = __builtin_bit_cast(float, w.x);
        o[1] = __builtin_bit_cast(float, w.y);
        o[2] = __builtin_bit_cast(float, w.z);
        o[3] = __builtin_bit_cast(float, w.w);
    } else {
        const unsigned words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; j++) { // (little endian: the element of the lower address in the lower half)
            o[2 * j] = (VT)__builtin_bit_cast(ST, (unsigned short)(words[j] & 0xFFFFu));
            o[2 * j + 1] = (VT)__builtin_bit_cast(ST, (unsigned short)(words[j] >> 16));
        }
    }
}

// the chain of the definition over one row of Q and one of K.  VEC: blocks of 32 bytes by 16-byte loads, the rest by elements.
// ST: the type the rows are stored in, VT unless the caller's pointers say otherwise (csr5_attention_lowp.hip: bf16 / fp16 rows, the
// chain in float); every element is widened by a cast, which is exact, and the chain runs c = 0, 1, 2, ... whatever the load width.
// HALVES (csr5_attention_bwd_drop_lowp.hip's bf16 kernels only): a 32-byte block is widened and consumed 16 bytes at a time, the
// accumulator pinned in a register between the halves, so that at most 8 + 8 widened elements are live next to the mask's hash
// instead of 16 + 16 -- the same FMAs in the same order, the same bits; without it those kernels spill under their 6-wave attribute
// 
template <typename VT, bool VEC, bool HALVES = false, typename ST>
__device__ __forceinline__ VT att_score(const ST *__restrict__ q, const ST *__restrict__ kr, const int k)
{
    constexpr int PER = 16 / (int)sizeof(ST);
    VT acc = (VT)0;
    int c = 0;
    if constexpr (VEC && HALVES) {
        for (; c + 2 * PER <= k; c += 2 * PER) {
#pragma unroll
            for (int half = 0; half < 2; half++) {
                VT a[PER], b[PER];
                att_load16<ST>(q + c + half * PER, a);
                att_load16<ST>(kr + c + half * PER, b);
#pragma unroll
                for (int j = 0; j < PER; j++)
                    acc = fma_vt(a[j], b[j], acc);
#if defined(__HIP_DEVICE_COMPILE__)
                asm volatile("" : "+v"(acc));
#endif
            }
        }
    } else if constexpr (VEC) {
        for (; c + 2 * PER <= k; c += 2 * PER) {
            VT a[2 * PER], b[2 * PER];
            att_load16<ST>(q + c, a);
            att_load16<ST>(q + c + PER, a + PER);
            att_load16<ST>(kr + c, b);
            att_load16<ST>(kr + c + PER, b + PER);
#pragma unroll
            for (int j = 0; j < 2 * PER; j++)
                acc = fma_vt(a[j], b[j], acc);
        }
    }
#pragma unroll 4
    for (; c < k; c++)
        acc = fma_vt((VT)q[c], (VT)kr[c], acc);
    return acc;
}

// The additive score bias of the biased entry points (csr5hip_mha_biased and its backward).  val: the value array, in tile order,
// of the handle whose pattern the kernel walks -- the parent's in the row kernels, the transposed companion's in the column
// kernel -- read at the storage position the entry's column is read from.  slopes: one value per head, or null (b = a, no
// multiplication).  c: the scale, converted once to the value type.
template <typename VT>
struct AttBias {
    const VT *val;
    const VT *slopes;
    VT c;
};

// the biased score of head h from the chain's qk and the entry's value a, every operation its own rounding:
// b = slope_h * a (one multiplication; b = a without slopes), s = fma(qk, c, b)
template <typename VT>
__device__ __forceinline__ VT att_bias_score(const AttBias<VT> &B, const int h, const VT qk, const VT a)
{
    const VT b = B.slopes ? B.slopes[h] * a : a;
    return fma_vt(qk, B.c, b);
}

// The additive score bias of the edge-bias entry points (csr5hip_mha_edge_bias and its backward): a caller-owned tensor in CSR
// order, element (e, h) at B[e * ldb + h], e the entry's CSR rank in the PARENT's pattern; null: b = +0 and nothing is read.
// map: null in the kernels that walk the parent's pattern, where an entry's position in the CSR order walked is its rank; in the
// column kernel the transposed companion's source map (position in A^T's CSR -> position in A's CSR).  c: the scale, converted
// once to the value type.  Nothing of the handle's values is read.
template <typename VT>
struct AttEdgeBias {
    const VT *B;
    const uint32_t *map;
    int ldb;
    VT c;
};

// the rank in the parent's CSR order of the entry at position q of the CSR order walked
template <typename VT>
__device__ __forceinline__ size_t att_edge_rank(const AttEdgeBias<VT> &E, const size_t q)
{
    return E.map ? (size_t)E.map[q] : q;
}

// the bias of head h of the entry of rank e
template <typename VT>
__device__ __forceinline__ VT att_edge_value(const AttEdgeBias<VT> &E, const size_t e, const int h)
{
    return E.B ? E.B[e * (size_t)E.ldb + (size_t)h] : (VT)0;
}

// the edge-biased score from the chain's qk and the entry's bias b: s = fma(qk, c, b), one rounding
template <typename VT>
__device__ __forceinline__ VT att_bias_score(const AttEdgeBias<VT> &E, const int, const VT qk, const VT b)
{
    return fma_vt(qk, E.c, b);
}

// The same for 16-bit operands (csr5hip_mha_lowp, csr5_attention_lowp.hip): B is stored in the operand type ST (bf16 or fp16) and
// widened exactly by the cast; c and the score are float.  The row kernels only: there is no map.
template <typename ST>
struct AttEdgeBiasLowp {
    const ST *B;
    int ldb;
    float c;
};

template <typename ST>
__device__ __forceinline__ float att_edge_value(const AttEdgeBiasLowp<ST> &E, const size_t e, const int h)
{
    return E.B ? (float)E.B[e * (size_t)E.ldb + (size_t)h] : 0.0f;
}

template <typename ST>
__device__ __forceinline__ float att_bias_score(const AttEdgeBiasLowp<ST> &E, const int, const float qk, const float b)
{
    return fma_vt(qk, E.c, b);
}

// Its sibling for the backward (csr5hip_mha_lowp_backward, csr5_attention_bwd_lowp.hip), whose column kernel needs the companion's
// source map as AttEdgeBias does.  A struct of its own: the forward's has no map and keeps its layout, and k_attention_lowp its
// kernarg block and its code.
template <typename ST>
struct AttEdgeBiasLowpMap {
    const ST *B;
    const uint32_t *map;
    int ldb;
    float c;
};

template <typename ST>
__device__ __forceinline__ size_t att_edge_rank(const AttEdgeBiasLowpMap<ST> &E, const size_t q)
{
    return E.map ? (size_t)E.map[q] : q;
}

template <typename ST>
__device__ __forceinline__ float att_edge_value(const AttEdgeBiasLowpMap<ST> &E, const size_t e, const int h)
{
    return E.B ? (float)E.B[e * (size_t)E.ldb + (size_t)h] : 0.0f;
}

template <typename ST>
__device__ __forceinline__ float att_bias_score(const AttEdgeBiasLowpMap<ST> &E, const int, const float qk, const float b)
{
    return fma_vt(qk, E.c, b);
}

// The additive score of csr5hip_gat and its backward (csr5_attention_gat.hip): the attention vector, head h's k values at a[h * k],
// or null (a = 1), and the negative slope of the LeakyReLU, converted once to the value type.  It rides NEXT TO an AttEdgeBias: the
// scale, B and the map are the edge call's.
template <typename VT>
struct AttGat {
    const VT *a;
    VT ns;
};

// u and l of one channel: u = q + k (one rounded addition, Q's element first on both sides of the backward), l = LeakyReLU(u)
template <typename VT>
__device__ __forceinline__ VT att_gat_leaky(const VT u, const VT ns)
{
    return u > (VT)0 ? u : ns * u;
}

// the chain of the definition over one row of Q and one of K: z = fma(a_c, l_c, z), c = 0, 1, 2, ..., from +0; a: that head's k
// values, or null (a = 1: fma(1, l, z) has the bits of z + l).  Element loads only: a 16-byte block would feed one addition each
template <typename VT>
__device__ __forceinline__ VT att_gat_z(const VT *__restrict__ q, const VT *__restrict__ kr, const VT *__restrict__ a, const VT ns,
                                        const int k)
{
    VT z = (VT)0;
    if (a) {
#pragma unroll 4
        for (int c = 0; c < k; c++)
            z = fma_vt(a[c], att_gat_leaky(q[c] + kr[c], ns), z);
    } else {
#pragma unroll 4
        for (int c = 0; c < k; c++)
            z = fma_vt((VT)1, att_gat_leaky(q[c] + kr[c], ns), z);
    }
    return z;
}

template <typename VT>
static void att_set_gat(AttGat<VT> &g, const AttCall &c)
{
    g.a = (const VT *)c.a;
    g.ns = (VT)c.negative_slope;
}

// The dropout mask of the dropped entry points (csr5hip_dropout.h; csr5_attention_drop.hip, csr5_attention_drop_gat.hip and their
// backwards): a pure function of (seed, offset, entry, head), so that the forward and both backward kernels recompute the same bits
// and nothing of length nnz is kept.  It rides NEXT TO an AttEdgeBias, whose map gives the column kernel the entry's rank.
//     counter = (e, g >> 2, offset low, offset high)    e: the entry's rank in the PARENT's CSR order, g = head0 + h
//     key     = (seed low, seed high)
//     dropped = philox4x32_10(counter, key)[g & 3] < thr
// thr = min(llrint(p 2^32), 2^32 - 1), cd = (VT)(1 / (1 - p)): formed once on the host (att_set_drop).  thr = 0 drops nothing.
struct AttDropKey {
    uint32_t thr;
    uint32_t seed_lo, seed_hi;
    uint32_t off_lo, off_hi;
    uint32_t head0; // the absolute head of head 0 of the operands (bwd_head moves it along with the slices); unsigned: no sum of it
                    // and a head index overflows (the host admits head0 + heads <= INT_MAX)
};
template <typename VT>
struct AttDrop {
    AttDropKey key;
    VT cd;
};

// Philox4x32-10 (Salmon et al., SC'11), the word w of the block of (c0, c1, c2, c3) under (k0, k1)
__host__ __device__ __forceinline__ uint32_t att_philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                             uint32_t k1, const int w)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
}

// whether head h (of the operands as K holds them) of the entry of rank e is kept
__host__ __device__ __forceinline__ bool att_drop_keep(const AttDropKey &K, const size_t e, const int h)
{
    const uint32_t g = K.head0 + (uint32_t)h;
    return att_philox_word((uint32_t)e, g >> 2, K.off_lo, K.off_hi, K.seed_lo, K.seed_hi, (int)(g & 3u)) >= K.thr;
}

// the factor of a kept weight in the backward: g_e = keep ? cd : +0
template <typename VT>
__device__ __forceinline__ VT att_drop_factor(const AttDrop<VT> &D, const size_t e, const int h)
{
    return att_drop_keep(D.key, e, h) ? D.cd : (VT)0;
}

inline AttDropKey att_drop_key(const AttCall &c)
{
    AttDropKey k;
    const long long t = llrint(c.p * 4294967296.0);
    k.thr = (uint32_t)(t < 0 ? 0 : t > 4294967295ll ? 4294967295ll : t);
    k.seed_lo = (uint32_t)c.seed;
    k.seed_hi = (uint32_t)(c.seed >> 32);
    k.off_lo = (uint32_t)c.offset;
    k.off_hi = (uint32_t)(c.offset >> 32);
    k.head0 = (uint32_t)c.head0;
    return k;
}

template <typename VT>
static void att_set_drop(AttDrop<VT> &d, const AttCall &c)
{
    d.key = att_drop_key(c);
    d.cd = (VT)(1.0 / (1.0 - c.p));
}

// The variant-specific part of a launch, forward and backward alike: the bias fields from the call.  side: the arrays of the pattern
// the kernel walks (the parent's, or the companion's in the column kernel); map: null where that pattern is the parent's, the
// companion's source map in the column kernel.
template <typename VT>
static void att_set_bias(AttBias<VT> &b, const DeviceArrays &side, const uint32_t *, const AttCall &c)
{
    b.val = (const VT *)side.val;
    b.slopes = (const VT *)c.slopes;
    b.c = (VT)c.scale;
}
template <typename VT>
static void att_set_bias(AttEdgeBias<VT> &b, const DeviceArrays &, const uint32_t *map, const AttCall &c)
{
    b.B = (const VT *)c.B;
    b.map = map;
    b.ldb = c.ldb;
    b.c = (VT)c.scale;
}
template <typename ST>
static void att_set_bias(AttEdgeBiasLowp<ST> &b, const DeviceArrays &, const uint32_t *, const AttCall &c)
{
    static_assert(sizeof(ST) == 2, "a 16-bit operand type");
    b.B = (const ST *)c.B;
    b.ldb = c.ldb;
    b.c = (float)c.scale;
}
template <typename ST>
static void att_set_bias(AttEdgeBiasLowpMap<ST> &b, const DeviceArrays &, const uint32_t *map, const AttCall &c)
{
    static_assert(sizeof(ST) == 2, "a 16-bit operand type");
    b.B = (const ST *)c.B;
    b.map = map;
    b.ldb = c.ldb;
    b.c = (float)c.scale;
}

// What a kernel stores of a computed value x: x itself where the storage type is the compute type; otherwise x rounded ONCE, to
// nearest even, by the cast.  The empty asm keeps x, a float, whole in a register first: without it the compiler folds the
// multiplication that produced x into the conversion (v_fma_mixlo_f16), which rounds the exact product to fp16 and skips the float
// rounding -- a different number where the float product is a tie of the narrow type, and not the definition's.
template <typename ST, typename VT>
__device__ __forceinline__ ST att_stored(VT x)
{
    if constexpr (sizeof(ST) != sizeof(VT)) {
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(x));
#endif
    }
    return (ST)x;
}

// LDS written by some lanes of a wavefront is read by others of the same wavefront
__device__ __forceinline__ void att_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the smallest power of two >= w, 1 <= w <= 64
__device__ __forceinline__ int att_pow2(const int w) { return w <= 1 ? 1 : 1 << (32 - __builtin_clz((unsigned)(w - 1))); }

} // namespace csr5
