// anonymouslib_hip.h -- host-only C++ front end of libcsr5hip.so (compiles with plain g++).
//
// Re-creates the reference's public surface so that a program written against
// CSR5_cuda/anonymouslib_cuda.h builds against this header unchanged:
//   template <iT, uiT, vT> class anonymouslibHandle      anonymouslib_cuda.h:11-53
//     anonymouslibHandle(m, n), warmup, inputCSR, asCSR, asCSR5, setX, spmv, destroy, setSigma
//   struct anonymouslib_timer { start(); stop() -> ms }  detail/cuda/utils_cuda.h:6-23
//   getB<iT, vT>(m, nnz), getFLOP<iT>(nnz)               detail/utils.h:10-20
//   ANONYMOUSLIB_* return codes / format ids / OMEGA / AUTO_TUNED_SIGMA
//                                                        detail/common.h:13-22, common_cuda.h:11-15
// Pointer semantics are the CUDA variant's: everything handed to inputCSR / setX / spmv is a DEVICE
// pointer owned by the caller (main.cu:43-63); asCSR5 permutes col_idx / val in place.
// Only <int, unsigned int, double> and <int, unsigned int, float> exist behind the C ABI; any other
// instantiation reports ANONYMOUSLIB_UNSUPPORTED_VALUE_TYPE from inputCSR.
#ifndef ANONYMOUSLIB_HIP_H
#define ANONYMOUSLIB_HIP_H

#include <sys/time.h>

#include <iostream>
#include <type_traits>

#include "csr5hip.h"

#define ANONYMOUSLIB_SUCCESS                   CSR5HIP_SUCCESS
#define ANONYMOUSLIB_UNKOWN_FORMAT             CSR5HIP_UNKOWN_FORMAT
#define ANONYMOUSLIB_UNSUPPORTED_CSR5_OMEGA    CSR5HIP_UNSUPPORTED_CSR5_OMEGA
#define ANONYMOUSLIB_CSR_TO_CSR5_FAILED        CSR5HIP_CSR_TO_CSR5_FAILED
#define ANONYMOUSLIB_UNSUPPORTED_CSR_SPMV      CSR5HIP_UNSUPPORTED_CSR_SPMV
#define ANONYMOUSLIB_UNSUPPORTED_VALUE_TYPE    CSR5HIP_UNSUPPORTED_VALUE_TYPE

#define ANONYMOUSLIB_FORMAT_CSR   CSR5HIP_FORMAT_CSR
#define ANONYMOUSLIB_FORMAT_CSR5  CSR5HIP_FORMAT_CSR5

#define ANONYMOUSLIB_CSR5_OMEGA        CSR5HIP_OMEGA
#define ANONYMOUSLIB_AUTO_TUNED_SIGMA  CSR5HIP_AUTO_TUNED_SIGMA

template <typename iT, typename vT>
double getB(const iT m, const iT nnz)
{
    // the reference CLI's byte model: x counted once per non-zero (detail/utils.h:10-14)
    return (double)(((double)m + 1 + nnz) * sizeof(iT) + (2.0 * nnz + m) * sizeof(vT));
}

template <typename iT>
double getFLOP(const iT nnz)
{
    return 2.0 * (double)nnz;
}

// Timer in milliseconds.  The CUDA variant's timer is a pair of events on the default stream whose stop() waits for the
// device (CSR5_cuda/detail/cuda/utils_cuda.h:6-23), so a caller may time an asynchronous spmv() loop without a
// synchronisation of its own.  Same guarantee here: start() and stop() drain the device before reading the host clock
// (the AVX2 variant's timer is plain gettimeofday, CSR5_avx2/detail/utils.h -- its spmv() is synchronous).
struct anonymouslib_timer {
    timeval t1, t2;
    void start()
    {
        (void)csr5hip_synchronize();
        gettimeofday(&t1, 0);
    }
    double stop()
    {
        (void)csr5hip_synchronize();
        gettimeofday(&t2, 0);
        return (t2.tv_sec - t1.tv_sec) * 1000.0 + (t2.tv_usec - t1.tv_usec) / 1000.0;
    }
};

template <class ANONYMOUSLIB_IT, class ANONYMOUSLIB_UIT, class ANONYMOUSLIB_VT>
class anonymouslibHandle
{
public:
    anonymouslibHandle(ANONYMOUSLIB_IT m, ANONYMOUSLIB_IT n) : _h(0), _err(ANONYMOUSLIB_SUCCESS), _quiet(false)
    {
        const bool ok_index = std::is_same<ANONYMOUSLIB_IT, int>::value &&
                              std::is_same<ANONYMOUSLIB_UIT, unsigned int>::value;
        int vt = std::is_same<ANONYMOUSLIB_VT, double>::value ? CSR5HIP_F64
               : std::is_same<ANONYMOUSLIB_VT, float>::value  ? CSR5HIP_F32 : -1;
        if (!ok_index || vt < 0)
            _err = ANONYMOUSLIB_UNSUPPORTED_VALUE_TYPE;
        else
            _err = csr5hip_create(&_h, (int)m, (int)n, vt);
    }
    ~anonymouslibHandle() { if (_h) csr5hip_free(_h); }

    int warmup() { return _h ? csr5hip_warmup(_h) : _err; }

    int inputCSR(ANONYMOUSLIB_IT nnz, ANONYMOUSLIB_IT *csr_row_pointer,
                 ANONYMOUSLIB_IT *csr_column_index, ANONYMOUSLIB_VT *csr_value)
    {
        if (!_h) return _err;
        return csr5hip_input_csr(_h, (int)nnz, (int32_t *)csr_row_pointer,
                                 (int32_t *)csr_column_index, (void *)csr_value);
    }

    int asCSR() { return _h ? csr5hip_as_csr(_h) : _err; }

    int asCSR5()
    {
        if (!_h) return _err;
        csr5hip_info before;
        csr5hip_get_info(_h, &before);
        const int err = csr5hip_as_csr5(_h);
        if (before.format == ANONYMOUSLIB_FORMAT_CSR && !_quiet) {
            // the stdout lines asCSR5 prints in the reference (anonymouslib_cuda.h:119,211-214)
            csr5hip_info i;
            csr5hip_get_info(_h, &i);
            std::cout << "omega = " << ANONYMOUSLIB_CSR5_OMEGA << ", sigma = " << i.sigma << ". " << std::endl;
            if (err == ANONYMOUSLIB_SUCCESS) {
                std::cout << "CSR->CSR5 malloc time = " << i.t_malloc_ms << " ms." << std::endl;
                std::cout << "CSR->CSR5 tile_ptr time = " << i.t_tile_ptr_ms << " ms." << std::endl;
                std::cout << "CSR->CSR5 tile_desc time = " << i.t_tile_desc_ms << " ms." << std::endl;
                std::cout << "CSR->CSR5 transpose time = " << i.t_transpose_ms << " ms." << std::endl;
            }
        }
        return err;
    }

    int setX(ANONYMOUSLIB_VT *x) { return _h ? csr5hip_set_x(_h, (const void *)x) : _err; }

    int spmv(const ANONYMOUSLIB_VT alpha, ANONYMOUSLIB_VT *y)
    {
        return _h ? csr5hip_spmv(_h, (double)alpha, (void *)y) : _err;
    }

    int destroy() { return _h ? csr5hip_destroy(_h) : _err; }

    void setSigma(int sigma) { if (_h) csr5hip_set_sigma(_h, sigma); }

    // ---- additions (not in the reference class) ----
    int spmv_repeat(const ANONYMOUSLIB_VT alpha, ANONYMOUSLIB_VT *y, int count)
    {
        return _h ? csr5hip_spmv_repeat(_h, (double)alpha, (void *)y, count) : _err;
    }
    // extension: Y = A * X for k dense vectors, row-major X (n x k, leading dimension ldx) and Y (m x k, ldy); device pointers
    int spmm(const ANONYMOUSLIB_VT *X, int ldx, int k, ANONYMOUSLIB_VT *Y, int ldy)
    {
        return _h ? csr5hip_spmm(_h, (const void *)X, ldx, k, (void *)Y, ldy) : _err;
    }
    // extension: Y[i, c] = the maximum (op = CSR5HIP_REDUCE_MAX) or minimum (CSR5HIP_REDUCE_MIN) over row i's stored entries e of
    // a_e * X[col(e), c] (weighted = 1) or of X[col(e), c] (weighted = 0), and arg[i, c] = the winning entry's CSR rank (-1 and +0 for
    // a row without entries); arg may be null; device pointers (csr5hip_reduce.h csr5hip_spmm_reduce)
    int spmmReduce(int op, int weighted, const ANONYMOUSLIB_VT *X, int ldx, int k, ANONYMOUSLIB_VT *Y, int ldy, int32_t *arg, int ldarg)
    {
        return _h ? csr5hip_spmm_reduce(_h, op, weighted, (const void *)X, ldx, k, (void *)Y, ldy, arg, ldarg) : _err;
    }
    // extension: its gradients from the forward's arg and dY (m x k): dX (n x k; needs buildTranspose) and, weighted only, dval (nnz
    // values in CSR order); either may be null (csr5hip_spmm_reduce_backward)
    int spmmReduceBackward(int weighted, const ANONYMOUSLIB_VT *X, int ldx, int k, const ANONYMOUSLIB_VT *dY, int lddy,
                           const int32_t *arg, int ldarg, ANONYMOUSLIB_VT *dX, int lddx, ANONYMOUSLIB_VT *dval)
    {
        return _h ? csr5hip_spmm_reduce_backward(_h, weighted, (const void *)X, ldx, k, (const void *)dY, lddy, arg, ldarg, (void *)dX,
                                                 lddx, (void *)dval)
                  : _err;
    }
    // extension: new values (nnz of them, CSR order, device pointer, not the array given to inputCSR) under the same pattern,
    // without a new conversion (csr5hip.h csr5hip_update_values)
    int updateValues(const ANONYMOUSLIB_VT *val) { return _h ? csr5hip_update_values(_h, (const void *)val) : _err; }
    // extension: products with the transpose (csr5hip.h csr5hip_build_transpose).  buildTranspose() once per conversion (allocates,
    // synchronises); then y = A^T x with x: m values, y: n values, and Y = A^T X with X: m x k, Y: n x k; device pointers
    int buildTranspose() { return _h ? csr5hip_build_transpose(_h) : _err; }
    int spmvT(const ANONYMOUSLIB_VT *x, ANONYMOUSLIB_VT *y) { return _h ? csr5hip_spmv_t(_h, (const void *)x, (void *)y) : _err; }
    int spmmT(const ANONYMOUSLIB_VT *X, int ldx, int k, ANONYMOUSLIB_VT *Y, int ldy)
    {
        return _h ? csr5hip_spmm_t(_h, (const void *)X, ldx, k, (void *)Y, ldy) : _err;
    }
    // extension: out[e] = dot(U[row(e), 0..k-1], V[col(e), 0..k-1]) for every stored element, nnz values in CSR order (the order
    // updateValues takes); U m x k (ldu), V n x k (ldv), row-major; device pointers; the matrix values play no part (csr5hip_sddmm)
    int sddmm(const ANONYMOUSLIB_VT *U, int ldu, const ANONYMOUSLIB_VT *V, int ldv, int k, ANONYMOUSLIB_VT *out)
    {
        return _h ? csr5hip_sddmm(_h, (const void *)U, ldu, (const void *)V, ldv, k, (void *)out) : _err;
    }
    // extension: attention on the pattern in one pass, O = softmax_row(Q K^T on the pattern) V with nothing of length nnz written and
    // the handle untouched; Q m x k (ldq), K n x k (ldk), V n x d (ldv), O m x d (ldo), row-major device pointers; EVERY row of O is
    // written in columns 0 .. d-1, rows without entries with +0 (csr5hip_attention)
    int attention(const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv,
                  int d, ANONYMOUSLIB_VT *O, int ldo)
    {
        return _h ? csr5hip_attention(_h, (const void *)Q, ldq, (const void *)K, ldk, k, (const void *)V, ldv, d, (void *)O, ldo)
                  : _err;
    }
    // extension: the gradients of attention's O for Q, K and V in two launches: dO m x d (lddo) in; dQ m x k, dK n x k, dV n x d out,
    // any of them null when not wanted, every row of a wanted one written; work: 4 m values of scratch, needed (as the transposed
    // companion, buildTranspose) only for dK or dV; the handle untouched (csr5hip_attention_backward)
    int attentionBackward(const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv,
                          int d, const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk,
                          ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work)
    {
        return _h ? csr5hip_attention_backward(_h, (const void *)Q, ldq, (const void *)K, ldk, k, (const void *)V, ldv, d,
                                               (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK, lddk, (void *)dV, lddv, (void *)work)
                  : _err;
    }
    // extension: attention for `heads` heads in one launch on packed operands: head h in columns h k .. h k + k of Q and K (ldq, ldk >=
    // heads k) and h d .. h d + d of V and O (ldv, ldo >= heads d); head h has the bits of attention on those slices (csr5hip_mha)
    int mha(int heads, const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv,
            int d, ANONYMOUSLIB_VT *O, int ldo)
    {
        return _h ? csr5hip_mha(_h, heads, (const void *)Q, ldq, (const void *)K, ldk, k, (const void *)V, ldv, d, (void *)O, ldo) : _err;
    }
    // extension: attentionBackward for `heads` heads in two launches on the packed layout (dO, dV as V; dQ, dK as Q); work: 4 m heads
    // values of scratch, needed (as the transposed companion) only for dK or dV (csr5hip_mha_backward)
    int mhaBackward(int heads, const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V,
                    int ldv, int d, const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk,
                    ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work)
    {
        return _h ? csr5hip_mha_backward(_h, heads, (const void *)Q, ldq, (const void *)K, ldk, k, (const void *)V, ldv, d,
                                         (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK, lddk, (void *)dV, lddv, (void *)work)
                  : _err;
    }
    // extension: mha on the scores fma(qk, scale, slopes[h] * a), a the handle's stored value of the entry (read, never written);
    // slopes: `heads` device values or null (csr5hip_mha_biased)
    int mhaBiased(int heads, double scale, const ANONYMOUSLIB_VT *slopes, const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K,
                  int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d, ANONYMOUSLIB_VT *O, int ldo)
    {
        return _h ? csr5hip_mha_biased(_h, heads, scale, (const void *)slopes, (const void *)Q, ldq, (const void *)K, ldk, k,
                                       (const void *)V, ldv, d, (void *)O, ldo)
                  : _err;
    }
    // extension: its gradients in two launches, operands as mhaBackward; dS (or null): nnz x heads values, the gradient for the biased
    // score of entry e (CSR order) and head h at dS[e ldds + h] (csr5hip_mha_biased_backward)
    int mhaBiasedBackward(int heads, double scale, const ANONYMOUSLIB_VT *slopes, const ANONYMOUSLIB_VT *Q, int ldq,
                          const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d, const ANONYMOUSLIB_VT *dO,
                          int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk, ANONYMOUSLIB_VT *dV, int lddv,
                          ANONYMOUSLIB_VT *work, ANONYMOUSLIB_VT *dS, int ldds)
    {
        return _h ? csr5hip_mha_biased_backward(_h, heads, scale, (const void *)slopes, (const void *)Q, ldq, (const void *)K, ldk, k,
                                                (const void *)V, ldv, d, (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK, lddk,
                                                (void *)dV, lddv, (void *)work, (void *)dS, ldds)
                  : _err;
    }
    // extension: mha on the scores fma(qk, scale, B[e ldb + h]), B the caller's nnz x heads device values in CSR order (e the entry's
    // CSR rank) or null for no bias; the handle's values are not read (csr5hip_mha_edge_bias)
    int mhaEdgeBias(int heads, double scale, const ANONYMOUSLIB_VT *B, int ldb, const ANONYMOUSLIB_VT *Q, int ldq,
                    const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d, ANONYMOUSLIB_VT *O, int ldo)
    {
        return _h ? csr5hip_mha_edge_bias(_h, heads, scale, (const void *)B, ldb, (const void *)Q, ldq, (const void *)K, ldk, k,
                                          (const void *)V, ldv, d, (void *)O, ldo)
                  : _err;
    }
    // extension: mhaEdgeBias on operands STORED in 16 bits -- operand_type CSR5HIP_BF16 or CSR5HIP_F16, whatever ANONYMOUSLIB_VT is; B, Q,
    // K, V and O device pointers to that type, leading dimensions in its elements -- computed in fp32, O rounded once (csr5hip_mha_lowp)
    int mhaLowp(int operand_type, int heads, double scale, const void *B, int ldb, const void *Q, int ldq, const void *K, int ldk, int k,
                const void *V, int ldv, int d, void *O, int ldo)
    {
        return _h ? csr5hip_mha_lowp(_h, operand_type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo) : _err;
    }
    // extension: mhaLowp's gradients in two launches -- B, Q, K, V, dO and the outputs dQ, dK, dV, dB device pointers to operand_type,
    // leading dimensions in its elements; work: 4 m heads FLOAT values whatever ANONYMOUSLIB_VT is; every output rounded once
    // (csr5hip_mha_lowp_backward)
    int mhaLowpBackward(int operand_type, int heads, double scale, const void *B, int ldb, const void *Q, int ldq, const void *K, int ldk,
                        int k, const void *V, int ldv, int d, const void *dO, int lddo, void *dQ, int lddq, void *dK, int lddk, void *dV,
                        int lddv, void *work, void *dB, int lddb)
    {
        return _h ? csr5hip_mha_lowp_backward(_h, operand_type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ, lddq,
                                              dK, lddk, dV, lddv, work, dB, lddb)
                  : _err;
    }
    // extension: mhaEdgeBias's gradients in two launches, operands as mhaBackward; dB (or null): nnz x heads values, the gradient of B, entry e
    // and head h at dB[e lddb + h] (csr5hip_mha_edge_bias_backward)
    int mhaEdgeBiasBackward(int heads, double scale, const ANONYMOUSLIB_VT *B, int ldb, const ANONYMOUSLIB_VT *Q, int ldq,
                            const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d,
                            const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk,
                            ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work, ANONYMOUSLIB_VT *dB, int lddb)
    {
        return _h ? csr5hip_mha_edge_bias_backward(_h, heads, scale, (const void *)B, ldb, (const void *)Q, ldq, (const void *)K, ldk,
                                                   k, (const void *)V, ldv, d, (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK,
                                                   lddk, (void *)dV, lddv, (void *)work, (void *)dB, lddb)
                  : _err;
    }
    // extension: additive (GAT, GATv2) attention: mhaEdgeBias with the score fma(sum_c a[h k + c] LeakyReLU(Q[i, h, c] + K[j, h, c]),
    // scale, B[e ldb + h]); a: heads k contiguous device values or null (a = 1); GAT is k = 1 without a (csr5hip_gat)
    int gat(int heads, double negative_slope, const ANONYMOUSLIB_VT *a, double scale, const ANONYMOUSLIB_VT *B, int ldb,
            const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d,
            ANONYMOUSLIB_VT *O, int ldo)
    {
        return _h ? csr5hip_gat(_h, heads, negative_slope, (const void *)a, scale, (const void *)B, ldb, (const void *)Q, ldq,
                                (const void *)K, ldk, k, (const void *)V, ldv, d, (void *)O, ldo)
                  : _err;
    }
    // extension: gat's gradients in two launches, operands and dB as mhaEdgeBiasBackward; dAr (or null): m x heads k values, the row's
    // share of the gradient of a, whose gradient is the sum of dAr over the rows (csr5hip_gat_backward)
    int gatBackward(int heads, double negative_slope, const ANONYMOUSLIB_VT *a, double scale, const ANONYMOUSLIB_VT *B, int ldb,
                    const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d,
                    const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk,
                    ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work, ANONYMOUSLIB_VT *dB, int lddb, ANONYMOUSLIB_VT *dAr, int lddar)
    {
        return _h ? csr5hip_gat_backward(_h, heads, negative_slope, (const void *)a, scale, (const void *)B, ldb, (const void *)Q, ldq,
                                         (const void *)K, ldk, k, (const void *)V, ldv, d, (const void *)dO, lddo, (void *)dQ, lddq,
                                         (void *)dK, lddk, (void *)dV, lddv, (void *)work, (void *)dB, lddb, (void *)dAr, lddar)
                  : _err;
    }
    // extension: mhaEdgeBias / gat and their backwards with a seeded dropout mask on the attention weights (csr5hip_dropout.h: the
    // mask's definition; p in [0, 1), seed and offset by value, head0 the absolute head of the operands' head 0), and the mask itself,
    // one byte per entry and head at mask[e ldm + h]
    int dropoutMha(int heads, double scale, const ANONYMOUSLIB_VT *B, int ldb, const ANONYMOUSLIB_VT *Q, int ldq,
                   const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d, ANONYMOUSLIB_VT *O, int ldo,
                   double p, unsigned long long seed, unsigned long long offset = 0, int head0 = 0)
    {
        return _h ? csr5hip_dropout_mha(_h, heads, scale, (const void *)B, ldb, (const void *)Q, ldq, (const void *)K, ldk, k,
                                        (const void *)V, ldv, d, (void *)O, ldo, p, seed, offset, head0)
                  : _err;
    }
    int dropoutMhaBackward(int heads, double scale, const ANONYMOUSLIB_VT *B, int ldb, const ANONYMOUSLIB_VT *Q, int ldq,
                           const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d,
                           const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK, int lddk,
                           ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work, ANONYMOUSLIB_VT *dB, int lddb, double p,
                           unsigned long long seed, unsigned long long offset = 0, int head0 = 0)
    {
        return _h ? csr5hip_dropout_mha_backward(_h, heads, scale, (const void *)B, ldb, (const void *)Q, ldq, (const void *)K, ldk, k,
                                                 (const void *)V, ldv, d, (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK, lddk,
                                                 (void *)dV, lddv, (void *)work, (void *)dB, lddb, p, seed, offset, head0)
                  : _err;
    }
    int dropoutGat(int heads, double negative_slope, const ANONYMOUSLIB_VT *a, double scale, const ANONYMOUSLIB_VT *B, int ldb,
                   const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V, int ldv, int d,
                   ANONYMOUSLIB_VT *O, int ldo, double p, unsigned long long seed, unsigned long long offset = 0, int head0 = 0)
    {
        return _h ? csr5hip_dropout_gat(_h, heads, negative_slope, (const void *)a, scale, (const void *)B, ldb, (const void *)Q, ldq,
                                        (const void *)K, ldk, k, (const void *)V, ldv, d, (void *)O, ldo, p, seed, offset, head0)
                  : _err;
    }
    int dropoutGatBackward(int heads, double negative_slope, const ANONYMOUSLIB_VT *a, double scale, const ANONYMOUSLIB_VT *B, int ldb,
                           const ANONYMOUSLIB_VT *Q, int ldq, const ANONYMOUSLIB_VT *K, int ldk, int k, const ANONYMOUSLIB_VT *V,
                           int ldv, int d, const ANONYMOUSLIB_VT *dO, int lddo, ANONYMOUSLIB_VT *dQ, int lddq, ANONYMOUSLIB_VT *dK,
                           int lddk, ANONYMOUSLIB_VT *dV, int lddv, ANONYMOUSLIB_VT *work, ANONYMOUSLIB_VT *dB, int lddb,
                           ANONYMOUSLIB_VT *dAr, int lddar, double p, unsigned long long seed, unsigned long long offset = 0,
                           int head0 = 0)
    {
        return _h ? csr5hip_dropout_gat_backward(_h, heads, negative_slope, (const void *)a, scale, (const void *)B, ldb,
                                                 (const void *)Q, ldq, (const void *)K, ldk, k, (const void *)V, ldv, d,
                                                 (const void *)dO, lddo, (void *)dQ, lddq, (void *)dK, lddk, (void *)dV, lddv,
                                                 (void *)work, (void *)dB, lddb, (void *)dAr, lddar, p, seed, offset, head0)
                  : _err;
    }
    // extension: dropoutMha / dropoutMhaBackward on operands STORED in 16 bits -- operand_type, the void * operands, their leading
    // dimensions and the FLOAT workspace as mhaLowp / mhaLowpBackward, the mask as dropoutMha; computed in fp32, every output rounded
    // once (csr5hip_dropout_lowp.h)
    int dropoutMhaLowp(int operand_type, int heads, double scale, const void *B, int ldb, const void *Q, int ldq, const void *K, int ldk,
                       int k, const void *V, int ldv, int d, void *O, int ldo, double p, unsigned long long seed,
                       unsigned long long offset = 0, int head0 = 0)
    {
        return _h ? csr5hip_dropout_mha_lowp(_h, operand_type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, O, ldo, p, seed,
                                             offset, head0)
                  : _err;
    }
    int dropoutMhaLowpBackward(int operand_type, int heads, double scale, const void *B, int ldb, const void *Q, int ldq, const void *K,
                               int ldk, int k, const void *V, int ldv, int d, const void *dO, int lddo, void *dQ, int lddq, void *dK,
                               int lddk, void *dV, int lddv, void *work, void *dB, int lddb, double p, unsigned long long seed,
                               unsigned long long offset = 0, int head0 = 0)
    {
        return _h ? csr5hip_dropout_mha_lowp_backward(_h, operand_type, heads, scale, B, ldb, Q, ldq, K, ldk, k, V, ldv, d, dO, lddo, dQ,
                                                      lddq, dK, lddk, dV, lddv, work, dB, lddb, p, seed, offset, head0)
                  : _err;
    }
    int dropoutMask(int heads, double p, unsigned long long seed, unsigned long long offset, int head0, unsigned char *mask, int ldm)
    {
        return _h ? csr5hip_dropout_mask(_h, heads, p, seed, offset, head0, (void *)mask, ldm) : _err;
    }
    // extension: softmax over the stored entries of every row and its gradient, nnz values in CSR order in and out (the order sddmm
    // writes and updateValues takes); device pointers; CSR and CSR5 format alike (csr5hip_row_softmax / csr5hip_row_softmax_grad)
    int rowSoftmax(const ANONYMOUSLIB_VT *scores, ANONYMOUSLIB_VT *out)
    {
        return _h ? csr5hip_row_softmax(_h, (const void *)scores, (void *)out) : _err;
    }
    int rowSoftmaxGrad(const ANONYMOUSLIB_VT *p, const ANONYMOUSLIB_VT *g, ANONYMOUSLIB_VT *out)
    {
        return _h ? csr5hip_row_softmax_grad(_h, (const void *)p, (const void *)g, (void *)out) : _err;
    }
    int autotuneSigma(ANONYMOUSLIB_VT *y, int *sigma = 0, double *us = 0)
    {
        return _h ? csr5hip_autotune_sigma(_h, (void *)y, sigma, us) : _err;
    }
    int setOption(int option, int value) { return _h ? csr5hip_set_option(_h, option, value) : _err; }
    void setQuiet(bool q) { _quiet = q; }
    csr5hip_handle native() const { return _h; }

private:
    anonymouslibHandle(const anonymouslibHandle &);
    anonymouslibHandle &operator=(const anonymouslibHandle &);
    csr5hip_handle _h;
    int _err;
    bool _quiet;
};

// One matrix on the G GPUs of a node (not in the reference, which is single-device: main.cu:25-26): same member
// names as anonymouslibHandle over csr5hip_multi_*.  inputCSR / setX take DEVICE pointers on devices[0]; y lives
// sharded on the devices (gatherY copies it to a host vector for checks).
template <class ANONYMOUSLIB_IT, class ANONYMOUSLIB_UIT, class ANONYMOUSLIB_VT>
class anonymouslibMultiHandle
{
public:
    anonymouslibMultiHandle(const int *devices, int ngpus, ANONYMOUSLIB_IT m, ANONYMOUSLIB_IT n) : _h(0)
    {
        const int vt = std::is_same<ANONYMOUSLIB_VT, double>::value ? CSR5HIP_F64
                     : std::is_same<ANONYMOUSLIB_VT, float>::value  ? CSR5HIP_F32 : -1;
        _err = vt < 0 ? ANONYMOUSLIB_UNSUPPORTED_VALUE_TYPE : csr5hip_multi_create(&_h, devices, ngpus, (int)m, (int)n, vt);
        _g = ngpus;
    }
    ~anonymouslibMultiHandle() { if (_h) csr5hip_multi_free(_h); }
    int inputCSR(ANONYMOUSLIB_IT nnz, ANONYMOUSLIB_IT *row_ptr, ANONYMOUSLIB_IT *col_idx, ANONYMOUSLIB_VT *val)
    {
        return _h ? csr5hip_multi_input_csr(_h, (int)nnz, (const int32_t *)row_ptr, (const int32_t *)col_idx, val) : _err;
    }
    void setSigma(int sigma) { if (_h) csr5hip_multi_set_sigma(_h, sigma); }
    int setOption(int option, int value) { return _h ? csr5hip_multi_set_option(_h, option, value) : _err; }
    int asCSR5()
    {
        if (!_h) return _err;
        const int err = csr5hip_multi_as_csr5(_h);
        for (int g = 0; g < _g && err == ANONYMOUSLIB_SUCCESS; g++) {
            csr5hip_shard s;
            csr5hip_info i;
            csr5hip_multi_shard(_h, g, &s);
            csr5hip_get_info(s.handle, &i);
            std::cout << "GPU shard " << g << " on device " << s.device << ": rows [" << s.row_lo << ", " << s.row_hi
                      << "), nnz = " << s.nnz << ", omega = " << ANONYMOUSLIB_CSR5_OMEGA << ", sigma = " << i.sigma
                      << ", tiles = " << i.p << std::endl;
        }
        return err;
    }
    int setX(ANONYMOUSLIB_VT *x) { return _h ? csr5hip_multi_set_x(_h, x) : _err; }
    int updateValues(const ANONYMOUSLIB_VT *val) { return _h ? csr5hip_multi_update_values(_h, (const void *)val) : _err; }
    int spmv(const ANONYMOUSLIB_VT alpha) { return _h ? csr5hip_multi_spmv(_h, (double)alpha) : _err; }
    int spmv_repeat(const ANONYMOUSLIB_VT alpha, int count) { return _h ? csr5hip_multi_spmv_repeat(_h, (double)alpha, count) : _err; }
    int synchronize() { return _h ? csr5hip_multi_synchronize(_h) : _err; }
    int gatherY(ANONYMOUSLIB_VT *host_y) { return _h ? csr5hip_multi_gather_y(_h, host_y) : _err; }
    int destroy() { return _h ? csr5hip_multi_destroy(_h) : _err; }
    csr5hip_multi native() const { return _h; }

private:
    anonymouslibMultiHandle(const anonymouslibMultiHandle &);
    anonymouslibMultiHandle &operator=(const anonymouslibMultiHandle &);
    csr5hip_multi _h;
    int _err, _g;
};

#endif // ANONYMOUSLIB_HIP_H
