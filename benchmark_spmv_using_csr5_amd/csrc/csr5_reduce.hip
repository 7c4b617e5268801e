// csr5_reduce.hip -- max / min aggregation on the CSR5 pattern for gfx950 (wave64), with its argmax and its two gradients:
//     Y[i, c] = max (or min) over the stored entries e of row i of  a_e * X[col(e), c]   (or of X[col(e), c], unweighted)
// The contract -- the order that makes the reduction total, the forward's bits, the gradients and the summation tree of dX -- is
// include/csr5hip_reduce.h; the kernel templates and the typed launchers are csr5_reduce_kern.h, which the host emulation compiles
// too.  No atomics, no workspace, nothing allocated: every launcher only enqueues.
#include "csr5_internal.h"
#include "csr5_wave.h"

// a product is one rounded multiplication, a chain's FMAs are written out (fma_vt); nothing else may be contracted
#pragma clang fp contract(off)

#include "csr5_reduce_kern.h"

namespace csr5 {

// The product build compiles this file once per value type (-DCSR5_REDUCE_ONLY_F64 / -DCSR5_REDUCE_ONLY_F32), as csr5_sddmm.hip.
#if !defined(CSR5_REDUCE_ONLY_F32)
hipError_t launch_spmm_reduce_f64(const Geometry &g, const DeviceArrays &d, int op, int weighted, const void *X, int ldx, int k, void *Y,
                                  int ldy, int32_t *arg, int ldarg, hipStream_t s)
{
    return reduce_typed<double>(g, d, op, weighted, X, ldx, k, Y, ldy, arg, ldarg, s);
}
hipError_t launch_spmm_reduce_dval_f64(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, const void *dY, int lddy,
                                       const int32_t *arg, int ldarg, void *dval, hipStream_t s)
{
    return reduce_dval_typed<double>(g, d, X, ldx, k, dY, lddy, arg, ldarg, dval, s);
}
hipError_t launch_spmm_reduce_dx_f64(const Geometry &gt, const DeviceArrays &dt, const uint32_t *map, int weighted, int k, const void *dY,
                                     int lddy, const int32_t *arg, int ldarg, void *dX, int lddx, hipStream_t s)
{
    return reduce_dx_typed<double>(gt, dt, map, weighted, k, dY, lddy, arg, ldarg, dX, lddx, s);
}
#endif
#if !defined(CSR5_REDUCE_ONLY_F64)
hipError_t launch_spmm_reduce_f32(const Geometry &g, const DeviceArrays &d, int op, int weighted, const void *X, int ldx, int k, void *Y,
                                  int ldy, int32_t *arg, int ldarg, hipStream_t s)
{
    return reduce_typed<float>(g, d, op, weighted, X, ldx, k, Y, ldy, arg, ldarg, s);
}
hipError_t launch_spmm_reduce_dval_f32(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, const void *dY, int lddy,
                                       const int32_t *arg, int ldarg, void *dval, hipStream_t s)
{
    return reduce_dval_typed<float>(g, d, X, ldx, k, dY, lddy, arg, ldarg, dval, s);
}
hipError_t launch_spmm_reduce_dx_f32(const Geometry &gt, const DeviceArrays &dt, const uint32_t *map, int weighted, int k, const void *dY,
                                     int lddy, const int32_t *arg, int ldarg, void *dX, int lddx, hipStream_t s)
{
    return reduce_dx_typed<float>(gt, dt, map, weighted, k, dY, lddy, arg, ldarg, dX, lddx, s);
}
#endif

#if !defined(CSR5_REDUCE_ONLY_F32)
hipError_t launch_spmm_reduce_f32(const Geometry &g, const DeviceArrays &d, int op, int weighted, const void *X, int ldx, int k, void *Y,
                                  int ldy, int32_t *arg, int ldarg, hipStream_t s);
hipError_t launch_spmm_reduce_dval_f32(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, const void *dY, int lddy,
                                       const int32_t *arg, int ldarg, void *dval, hipStream_t s);
hipError_t launch_spmm_reduce_dx_f32(const Geometry &gt, const DeviceArrays &dt, const uint32_t *map, int weighted, int k, const void *dY,
                                     int lddy, const int32_t *arg, int ldarg, void *dX, int lddx, hipStream_t s);

hipError_t launch_spmm_reduce(const Geometry &g, const DeviceArrays &d, int value_type, int op, int weighted, const void *X, int ldx,
                              int k, void *Y, int ldy, int32_t *arg, int ldarg, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_spmm_reduce_f64(g, d, op, weighted, X, ldx, k, Y, ldy, arg, ldarg, s)
                                     : launch_spmm_reduce_f32(g, d, op, weighted, X, ldx, k, Y, ldy, arg, ldarg, s);
}
hipError_t launch_spmm_reduce_dval(const Geometry &g, const DeviceArrays &d, int value_type, const void *X, int ldx, int k,
                                   const void *dY, int lddy, const int32_t *arg, int ldarg, void *dval, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_spmm_reduce_dval_f64(g, d, X, ldx, k, dY, lddy, arg, ldarg, dval, s)
                                     : launch_spmm_reduce_dval_f32(g, d, X, ldx, k, dY, lddy, arg, ldarg, dval, s);
}
hipError_t launch_spmm_reduce_dx(const Geometry &gt, const DeviceArrays &dt, const uint32_t *map, int value_type, int weighted, int k,
                                 const void *dY, int lddy, const int32_t *arg, int ldarg, void *dX, int lddx, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_spmm_reduce_dx_f64(gt, dt, map, weighted, k, dY, lddy, arg, ldarg, dX, lddx, s)
                                     : launch_spmm_reduce_dx_f32(gt, dt, map, weighted, k, dY, lddy, arg, ldarg, dX, lddx, s);
}
#endif

} // namespace csr5
