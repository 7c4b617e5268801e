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

// the row classes' constants, the rank -> storage map and the score chain (csr5_attention_dev.h, shared with the backward) and the
// kernel templates (csr5_attention_kern.h, shared with the biased entry point's translation unit csr5_attention_bias.hip)
#include "csr5_attention_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher as well.
#if !defined(CSR5_ATTENTION_ONLY_F32)
extern template AttLaunch attention_launch<AttArgs<float>>;
template AttLaunch attention_launch<AttArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
// heads == 1 is the single-head call: k_attention<VT, VEC, false>
hipError_t launch_mha(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttArgs<double>>(g, d, c, s);
    return attention_launch<AttArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
