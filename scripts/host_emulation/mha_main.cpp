// Stand-alone CPU run of csr5_attention.hip's multi-head entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file
// written by run_mha.py (header, row_ptr, tile-ordered columns, tile_ptr, packed Q, K, V), writes O.  heads > 0: launch_mha with
// that many heads and `groups` head groups (0: the rule).  heads = 0: the single-head call (launch_mha, one head) on the slices that start
// offk / offd columns into the same rows.  Every array is a heap block of its exact size, so -fsanitize=address sees any access
// outside it.
#include "csr5_attention.hip"
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[16];
    if (!f || fread(h, 4, 16, f) != 16) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], k = h[5], d = h[6], ldq = h[7], ldk = h[8], ldv = h[9], ldo = h[10], f64 = h[11];
    const int heads = h[12], groups = h[13], offk = h[14], offd = h[15];
    const size_t s = f64 ? 8 : 4;
    int32_t *rp = (int32_t *)malloc(4 * (size_t)(m + 1)), *col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    uint32_t *tp = (uint32_t *)malloc(4 * (size_t)(p + 1));
    auto block = [&](int rows, int ld) { return (char *)malloc(s * (size_t)rows * ld + (ld ? 0 : 8)); };
    char *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *O = block(m, ldo);
    size_t got = fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f);
    fclose(f);
    memset(O, 0xFF, s * (size_t)m * ldo); // NaN poison
    csr5::Geometry g{};
    g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
    csr5::DeviceArrays da{};
    da.row_ptr = rp; da.col = col; da.tile_ptr = tp;
    const int vt = f64 ? CSR5HIP_F64 : CSR5HIP_F32;
    csr5::AttCall c{};
    c.k = k; c.d = d; c.ldq = ldq; c.ldk = ldk; c.ldv = ldv; c.ldo = ldo;
    if (heads > 0) {
        c.heads = heads; c.groups = groups; c.Q = Q; c.K = K; c.V = V; c.O = O;
    } else { // the single-head call on one head's slices
        c.heads = 1; c.Q = Q + s * offk; c.K = K + s * offk; c.V = V + s * offd; c.O = O + s * offd;
    }
    const int rc = csr5::launch_mha(g, da, vt, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(O, s, (size_t)m * ldo, f);
    fclose(f);
    free(rp); free(col); free(tp); free(Q); free(K); free(V); free(O);
    return rc;
}
