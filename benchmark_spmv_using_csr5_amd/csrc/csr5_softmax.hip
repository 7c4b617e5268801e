// csr5_softmax.hip -- softmax over the stored entries of every row ("edge softmax") and its gradient, for gfx950 (wave64).
// Both work on arrays of nnz values in CSR ORDER (the order inputCSR's value array had, sddmm writes, update_values reads):
//
//     forward    out[e] = exp(s[e] - M_r) / Z_r        M_r = max of the row's scores, Z_r = sum over the row of exp(s[j] - M_r)
//     gradient   out[e] = p[e] * (g[e] - D_r)          D_r = sum over the row of p[j] * g[j]
//
// row(e) comes from row_ptr, and row_ptr is ALL that is read of the matrix: no columns, no values, no x, no tile structure, no
// kernel table.  The calls are therefore the same in CSR and in CSR5 format.  No workspace, no pre-pass, nothing read back.
//
// DEFINITION (what the error bound of tests/softmax_reference.py is derived from).  M is the exact maximum of the row (NaN
// entries are skipped by the maximum and then poison the sum).  A term is ONE subtraction and ONE exponential of the device
// library (exp / expf at full precision, subnormal results kept).  Z is summed by the tree below.  The quotient is ONE
// reciprocal per row, r = 1 / Z (a correctly rounded division), and ONE multiplication per entry, out = term * r.  The gradient
// rounds every product p[j] * g[j], sums them by the same tree, then rounds g[e] - D and the product with p[e]: nothing is
// contracted into a fused multiply-add (fp contract(off)).  No running maximum is rescaled.
//
// NON-FINITE values behave as in torch.softmax: a -Inf score gets exactly +0 (exp(-Inf) = +0, times r); a row that holds a NaN
// or a +Inf (Inf - Inf = NaN) or only -Inf (-Inf - -Inf = NaN) gets NaN in every entry, through Z, and no other row does: a row
// is computed from its own entries only (padding lanes contribute +0 through a select, never through arithmetic on foreign data).
// Empty rows write nothing.  A finite row of one entry gives exp(0) * (1 / 1) = 1 exactly.
//
// ROW CLASSES, decided per row on the device from L = row_ptr[r + 1] - row_ptr[r]; a workgroup of 256 lanes owns 256 consecutive
// rows, every wavefront 64 of them (lane l holds the bounds of row l):
//     L <= 4            4 lanes per row, 16 rows of the wavefront per pass
//     5 <= L <= 16      16 lanes per row, 4 rows per pass
//     17 <= L <= 512    one row at a time with all 64 lanes (ballot loop), <= 8 entries per lane in registers: read once,
//                       written once
//     L > 512           listed in LDS and, after a barrier, walked by the four wavefronts together: up to 2 048 entries in
//                       registers (read once, written once); beyond that three sweeps (maximum, sum, write; the gradient two)
//
// THE TREE of Z and of D depends on L and on nothing else:
//     L <= 512          slot(j) = j mod 64.  Every slot sums its terms j = slot, slot + 64, slot + 128, ... in ascending order
//                       onto +0; the 64 slot sums (+0 for a slot without terms) are added by the balanced binary tree over
//                       adjacent slots: pairs (0,1) (2,3) ..., then quads, ... , then the two halves.  Rows of at most 4 (16)
//                       entries run the leading sub-tree over 4 (16) slots: adding +0 is exact, so that is the same tree.
//     L > 512           slot(j) = j mod 256, summed per slot as above; slots 64 w .. 64 w + 63 by the balanced tree
//                       (wavefront w), then (w0 + w1) + (w2 + w3).
//
// DETERMINISM CONTRACT.  The bits of a row's outputs depend only on that row's inputs (values and order) and on the value type:
// not on sigma, any option or the format, not on pointer alignment (element loads only), not on m, nnz or the position of the
// row in the matrix, not on what neighbouring rows hold, not on the run.  No atomics on values, no scratch.
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every operation of the definition is its own rounding
#pragma clang fp contract(off)

namespace csr5 {

constexpr int SM_BLOCK = 256;                 // lanes = rows of a workgroup
constexpr int SM_WAVES = SM_BLOCK / OMEGA;
constexpr int SM_QUAD_ROW = 4;                // rows up to this many entries: 4 lanes per row
constexpr int SM_ROW16 = 16;                  // ... up to this many: 16 lanes per row
constexpr int SM_REGS = 8;                    // entries of a row a lane keeps in registers
constexpr int SM_WAVE_ROW = OMEGA * SM_REGS;  // rows up to 512 entries: one wavefront, in registers
constexpr int SM_BLOCK_REG_ROW = SM_BLOCK * SM_REGS; // rows up to 2 048 entries: the workgroup, in registers; beyond: sweeps

// ---- rows of at most G entries (and more than LO): G lanes per row, 64 / G rows of the wavefront per pass -----------------
template <typename VT, bool GRAD, int G, int LO>
__device__ __forceinline__ void softmax_short(const int a, const int len, const VT *__restrict__ in, const VT *__restrict__ gin,
                                              VT *__restrict__ out)
{
    constexpr int ROWS = OMEGA / G; // rows per pass
    const int lane = threadIdx.x & (OMEGA - 1);
    const int sub = lane / G, pos = lane % G;
    const unsigned long long cls = __ballot(len > LO && len <= G);
    if (!cls)
        return;
    for (int pass = 0; pass < G; pass++) {
        const unsigned long long here = (cls >> (pass * ROWS)) & ((1ull << ROWS) - 1);
        if (!here) // (wave-uniform)
            continue;
        const int src = pass * ROWS + sub;
        const int ra = __shfl(a, src, OMEGA);
        const int rl = __shfl(len, src, OMEGA);
        const bool act = ((cls >> src) & 1) && pos < rl;
        const size_t e = (size_t)ra + pos;
        if constexpr (!GRAD) {
            const VT s = act ? in[e] : neg_inf<VT>();
            const VT mx = group_max<G>(s);
            const VT t = act ? exp_vt(s - mx) : (VT)0;
            const VT r = (VT)1 / group_sum<G>(t);
            if (act)
                out[e] = t * r;
        } else {
            const VT p = act ? in[e] : (VT)0;
            const VT g = act ? gin[e] : (VT)0;
            const VT pg = p * g;
            const VT dsum = group_sum<G>(act ? pg : (VT)0);
            if (act)
                out[e] = p * (g - dsum);
        }
    }
}

// ---- a row of at most STRIDE x SM_REGS entries in registers: STRIDE = 64 one wavefront, STRIDE = 256 the workgroup ----------
template <typename VT, bool GRAD, int STRIDE>
__device__ __forceinline__ void softmax_in_regs(const int ra, const int rl, const int slot, const VT *__restrict__ in,
                                                const VT *__restrict__ gin, VT *__restrict__ out, VT *red)
{
    const VT *ip = in + (size_t)ra + slot;
    VT *op = out + (size_t)ra + slot;
    VT v[SM_REGS];
    if constexpr (!GRAD) {
        VT mx = neg_inf<VT>();
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            v[k] = neg_inf<VT>();
            if (k * STRIDE < rl) { // (uniform)
                if (k * STRIDE + slot < rl)
                    v[k] = ip[k * STRIDE];
                mx = max_vt(mx, v[k]);
            }
        }
        mx = wave_max(mx);
        if constexpr (STRIDE > OMEGA)
            mx = block_combine<VT, true>(mx, red);
        VT acc = (VT)0;
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            if (k * STRIDE < rl) {
                const VT t = exp_vt(v[k] - mx);
                v[k] = k * STRIDE + slot < rl ? t : (VT)0;
                acc += v[k];
            }
        }
        acc = wave_sum(acc);
        if constexpr (STRIDE > OMEGA)
            acc = block_combine<VT, false>(acc, red);
        const VT r = (VT)1 / acc;
#pragma unroll
        for (int k = 0; k < SM_REGS; k++)
            if (k * STRIDE + slot < rl)
                op[k * STRIDE] = v[k] * r;
    } else {
        const VT *gp = gin + (size_t)ra + slot;
        VT g[SM_REGS];
        VT acc = (VT)0;
#pragma unroll
        for (int k = 0; k < SM_REGS; k++) {
            v[k] = (VT)0;
            g[k] = (VT)0;
            if (k * STRIDE < rl) {
                const bool ok = k * STRIDE + slot < rl;
                if (ok) {
                    v[k] = ip[k * STRIDE];
                    g[k] = gp[k * STRIDE];
                }
                const VT pg = v[k] * g[k];
                acc += ok ? pg : (VT)0;
            }
        }
        acc = wave_sum(acc);
        if constexpr (STRIDE > OMEGA)
            acc = block_combine<VT, false>(acc, red);
#pragma unroll
        for (int k = 0; k < SM_REGS; k++)
            if (k * STRIDE + slot < rl)
                op[k * STRIDE] = v[k] * (g[k] - acc);
    }
}

// ---- a row beyond 2 048 entries: the workgroup sweeps it (maximum, sum, write; the gradient: sum, write) --------------------
template <typename VT, bool GRAD>
__device__ __forceinline__ void softmax_sweeps(const int ra, const int rl, const VT *__restrict__ in, const VT *__restrict__ gin,
                                               VT *__restrict__ out, VT *red)
{
    const int slot = (int)threadIdx.x;
    const VT *ip = in + (size_t)ra;
    VT *op = out + (size_t)ra;
    if constexpr (!GRAD) {
        VT mx = neg_inf<VT>();
        for (int j = slot; j < rl; j += SM_BLOCK)
            mx = max_vt(mx, ip[j]);
        mx = block_combine<VT, true>(wave_max(mx), red);
        VT acc = (VT)0;
        for (int j = slot; j < rl; j += SM_BLOCK)
            acc += exp_vt(ip[j] - mx);
        acc = block_combine<VT, false>(wave_sum(acc), red);
        const VT r = (VT)1 / acc;
        for (int j = slot; j < rl; j += SM_BLOCK)
            op[j] = exp_vt(ip[j] - mx) * r; // (the same subtraction and exponential as in the sum: the same term)
    } else {
        const VT *gp = gin + (size_t)ra;
        VT acc = (VT)0;
        for (int j = slot; j < rl; j += SM_BLOCK)
            acc += ip[j] * gp[j];
        acc = block_combine<VT, false>(wave_sum(acc), red);
        for (int j = slot; j < rl; j += SM_BLOCK)
            op[j] = ip[j] * (gp[j] - acc);
    }
}

// in: the scores (forward) or p (gradient); gin: g (gradient only)
template <typename VT, bool GRAD>
__global__ void __launch_bounds__(SM_BLOCK)
k_row_softmax(const int m, const int32_t *__restrict__ row_ptr, const VT *__restrict__ in, const VT *__restrict__ gin,
              VT *__restrict__ out)
{
    __shared__ int hub_n;
    __shared__ int hub_row[SM_BLOCK];
    __shared__ VT red[SM_WAVES];
    if (threadIdx.x == 0)
        hub_n = 0;
    __syncthreads();

    const int lane = threadIdx.x & (OMEGA - 1);
    const long long r = (long long)blockIdx.x * SM_BLOCK + threadIdx.x;
    int a = 0, len = 0;
    if (r < m) {
        a = row_ptr[r];
        len = row_ptr[r + 1] - a;
        len = len < 0 ? 0 : len;
    }
    softmax_short<VT, GRAD, SM_QUAD_ROW, 0>(a, len, in, gin, out);
    softmax_short<VT, GRAD, SM_ROW16, SM_QUAD_ROW>(a, len, in, gin, out);

    unsigned long long todo = __ballot(len > SM_ROW16 && len <= SM_WAVE_ROW);
    while (todo) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int ra = __builtin_amdgcn_readlane(a, src);
        const int rl = __builtin_amdgcn_readlane(len, src);
        softmax_in_regs<VT, GRAD, OMEGA>(ra, rl, lane, in, gin, out, red);
    }

    if (len > SM_WAVE_ROW)
        hub_row[atomicAdd(&hub_n, 1)] = (int)threadIdx.x; // (an integer counter in LDS: the order of the list decides no bit)
    __syncthreads();
    const int hubs = __builtin_amdgcn_readfirstlane(hub_n);
    for (int i = 0; i < hubs; i++) { // (uniform over the workgroup: the barriers inside are reached by all)
        const long long hr = (long long)blockIdx.x * SM_BLOCK + __builtin_amdgcn_readfirstlane(hub_row[i]);
        const int ra = __builtin_amdgcn_readfirstlane(row_ptr[hr]);
        const int rl = __builtin_amdgcn_readfirstlane(row_ptr[hr + 1]) - ra;
        if (rl <= SM_BLOCK_REG_ROW)
            softmax_in_regs<VT, GRAD, SM_BLOCK>(ra, rl, (int)threadIdx.x, in, gin, out, red);
        else
            softmax_sweeps<VT, GRAD>(ra, rl, in, gin, out, red);
    }
}

template <typename VT>
static hipError_t row_softmax_typed(int m, const int32_t *row_ptr, const void *in, const void *gin, void *out, bool grad, hipStream_t s)
{
    if (m <= 0)
        return hipSuccess;
    const dim3 grid((unsigned)(((long long)m + SM_BLOCK - 1) / SM_BLOCK)), block(SM_BLOCK);
    if (grad)
        hipLaunchKernelGGL((k_row_softmax<VT, true>), grid, block, 0, s, m, row_ptr, (const VT *)in, (const VT *)gin, (VT *)out);
    else
        hipLaunchKernelGGL((k_row_softmax<VT, false>), grid, block, 0, s, m, row_ptr, (const VT *)in, (const VT *)nullptr, (VT *)out);
    return hipGetLastError();
}

// The product build compiles this file once per value type (-DCSR5_SOFTMAX_ONLY_F64 / -DCSR5_SOFTMAX_ONLY_F32), as csr5_sddmm.hip.
#if !defined(CSR5_SOFTMAX_ONLY_F32)
hipError_t launch_row_softmax_f64(int m, const int32_t *row_ptr, const void *in, const void *gin, void *out, bool grad, hipStream_t s)
{
    return row_softmax_typed<double>(m, row_ptr, in, gin, out, grad, s);
}
#endif
#if !defined(CSR5_SOFTMAX_ONLY_F64)
hipError_t launch_row_softmax_f32(int m, const int32_t *row_ptr, const void *in, const void *gin, void *out, bool grad, hipStream_t s)
{
    return row_softmax_typed<float>(m, row_ptr, in, gin, out, grad, s);
}
#endif

#if !defined(CSR5_SOFTMAX_ONLY_F32)
hipError_t launch_row_softmax_f32(int m, const int32_t *row_ptr, const void *in, const void *gin, void *out, bool grad, hipStream_t s);

hipError_t launch_row_softmax(int m, const int32_t *row_ptr, int value_type, const void *scores, void *out, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_row_softmax_f64(m, row_ptr, scores, nullptr, out, false, s)
                                     : launch_row_softmax_f32(m, row_ptr, scores, nullptr, out, false, s);
}
hipError_t launch_row_softmax_grad(int m, const int32_t *row_ptr, int value_type, const void *p, const void *g, void *out,
                                   hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_row_softmax_f64(m, row_ptr, p, g, out, true, s)
                                     : launch_row_softmax_f32(m, row_ptr, p, g, out, true, s);
}
#endif

} // namespace csr5
