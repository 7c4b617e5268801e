// csr5_attention_gat.hip -- csr5hip_gat: additive (GAT, GATv2) attention on the pattern in ONE launch, for gfx950 (wave64).  The
// score of a stored entry e = (i, j) and head h is not a dot product: the non-linearity sits inside it,
//
//     u_c   = Q[i, h, c] + K[j, h, c]                 one rounded addition
//     l_c   = u_c > 0 ? u_c : ns * u_c                ns: negative_slope, converted once to the value type
//     z     = fma(a[h, c], l_c, z), c = 0, 1, 2, ...  from +0; a null: a = 1 (fma(1, l, z), the bits of z + l)
//     s_e,h = fma(z, c, B[e * ldb + h])               csr5_attention_edge.hip's rule: c the scale, B null: +0
//
// and EVERYTHING after the score is csr5_attention.hip's, per head, with these scores: M, w, Z and its tree, the normalisation after
// the product, the row classes, the summation orders, +0 for empty rows, the head groups.  GAT is k = 1 without a
// (s = LeakyReLU(el[i, h] + er[j, h])), GATv2 k = the feature width with a (heads, k).  These are the same kernel templates
// (csr5_attention_kern.h) instantiated with an argument struct derived from the edge one that carries a and ns (AttGatArgs:
// ARGS::GAT swaps att_score for att_gat_z); no other instantiation is touched by it.
//
// THE CHAIN takes element loads: a 16-byte block of Q and K would feed one addition per element, and GAT's k is 1.  a[h, :] is read
// by every entry of head h, through the scalar cache where the compiler proves it uniform.  B is read as the edge call reads it.
// THE HANDLE'S VALUES ARE NOT READ.
//
// NON-FINITE: a NaN in u fails u > 0 and stays a NaN through ns * u; otherwise as csr5_attention_edge.hip (a -Inf bias masks).
#include "csr5_internal.h"
#include "csr5_wave.h"

#include <math.h>

// every FMA is written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_attention_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_ATTENTION_ONLY_F64 / _F32), as csr5_sddmm.hip:
// each object holds the shared launcher's instantiation on its type, the fp64 one the dispatcher as well.
#if !defined(CSR5_ATTENTION_ONLY_F32)
extern template AttLaunch attention_launch<AttGatArgs<float>>;
template AttLaunch attention_launch<AttGatArgs<double>>;
#endif
#if !defined(CSR5_ATTENTION_ONLY_F64)
template AttLaunch attention_launch<AttGatArgs<float>>;
#endif

#if !defined(CSR5_ATTENTION_ONLY_F32)
hipError_t launch_gat(const Geometry &g, const DeviceArrays &d, int value_type, const AttCall &c, hipStream_t s)
{
    if (value_type == CSR5HIP_F64)
        return attention_launch<AttGatArgs<double>>(g, d, c, s);
    return attention_launch<AttGatArgs<float>>(g, d, c, s);
}
#endif

} // namespace csr5
