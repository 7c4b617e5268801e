// Stand-alone CPU run of csr5_attention_bwd.hip's multi-head entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case
// file written by run_mha.py (header; row_ptr, tile-ordered columns and tile_ptr of the matrix and of its transpose; packed Q, K,
// V, dO), writes dQ, dK, dV.  heads > 0: launch_mha_bwd with that many heads and `groups` head groups (0: the rule) and a
// workspace of exactly 4 m heads values.  heads = 0: the single-head call (launch_mha_bwd, one head) on the slices that start offk / offd
// columns into the same rows, with a workspace of 4 m values.  Every array is a heap block of its exact size.
#include "csr5_attention_bwd.hip"
#include <cstdlib>
struct Pattern {
    int32_t *rp, *col;
    uint32_t *tp;
    csr5::Geometry g{};
    csr5::DeviceArrays da{};
    size_t read(FILE *f, int m, int n, int nnz, int sigma, int p)
    {
        rp = (int32_t *)malloc(4 * (size_t)(m + 1));
        col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
        tp = (uint32_t *)malloc(4 * (size_t)(p + 1));
        g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
        da.row_ptr = rp; da.col = col; da.tile_ptr = tp;
        return fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f);
    }
    void release() { free(rp); free(col); free(tp); }
};
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[22];
    if (!f || fread(h, 4, 22, f) != 22) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], sigma_t = h[5], p_t = h[6], k = h[7], d = h[8];
    const int ldq = h[9], ldk = h[10], ldv = h[11], lddo = h[12], lddq = h[13], lddk = h[14], lddv = h[15], f64 = h[16], want = h[17];
    const int heads = h[18], groups = h[19], offk = h[20], offd = h[21];
    const size_t s = f64 ? 8 : 4;
    Pattern A, At;
    size_t got = A.read(f, m, n, nnz, sigma, p) + At.read(f, n, m, nnz, sigma_t, p_t);
    auto block = [&](int rows, int ld) { return (char *)malloc(s * (size_t)rows * ld + (ld ? 0 : 8)); };
    const size_t wn = 4 * (size_t)m * (heads > 0 ? heads : 1);
    char *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *dO = block(m, lddo);
    char *dQ = block(m, lddq), *dK = block(n, lddk), *dV = block(n, lddv), *work = (char *)malloc(s * wn + 8);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f) + fread(dO, s, (size_t)m * lddo, f);
    fclose(f);
    memset(dQ, 0xFF, s * (size_t)m * lddq); // NaN poison
    memset(dK, 0xFF, s * (size_t)n * lddk);
    memset(dV, 0xFF, s * (size_t)n * lddv);
    memset(work, 0xFF, s * wn);
    const bool column = want & 6;
    const int vt = f64 ? CSR5HIP_F64 : CSR5HIP_F32;
    const csr5::Geometry *gt = column ? &At.g : nullptr;
    const csr5::DeviceArrays *dt = column ? &At.da : nullptr;
    csr5::AttBwdCall c{};
    c.k = k; c.d = d; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.lddo = lddo; c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
    c.work = column ? work : nullptr; c.gt = gt; c.dt = dt;
    const size_t ok = heads > 0 ? 0 : s * offk, od = heads > 0 ? 0 : s * offd; // heads <= 0: the single-head call on one head's slices
    c.heads = heads > 0 ? heads : 1; c.groups = heads > 0 ? groups : 0;
    c.Q = Q + ok; c.K = K + ok; c.V = V + od; c.dO = dO + od;
    c.dQ = want & 1 ? dQ + ok : nullptr; c.dK = want & 2 ? dK + ok : nullptr; c.dV = want & 4 ? dV + od : nullptr;
    const int rc = csr5::launch_mha_bwd(A.g, A.da, vt, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(dQ, s, (size_t)m * lddq, f);
    fwrite(dK, s, (size_t)n * lddk, f);
    fwrite(dV, s, (size_t)n * lddv, f);
    fclose(f);
    A.release(); At.release();
    free(Q); free(K); free(V); free(dO); free(dQ); free(dK); free(dV); free(work);
    return rc;
}
