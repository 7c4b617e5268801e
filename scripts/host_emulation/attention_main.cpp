// Stand-alone CPU run of csr5_attention.hip on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file written by
// run_attention.py (header, row_ptr, tile-ordered columns, tile_ptr, Q, K, V), writes O.  Every array is a heap block of its exact
// size, so -fsanitize=address sees any access outside it.
#include "csr5_attention.hip"
#include <cstdlib>
int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int h[12];
    if (fread(h, 4, 12, f) != 12) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], k = h[5], d = h[6], ldq = h[7], ldk = h[8], ldv = h[9], ldo = h[10], f64 = h[11];
    const size_t s = f64 ? 8 : 4;
    // exact-size heap blocks: the address sanitizer sees any access outside them
    int32_t *rp = (int32_t *)malloc(4 * (m + 1)), *col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    uint32_t *tp = (uint32_t *)malloc(4 * (p + 1));
    char *Q = (char *)malloc(s * (size_t)m * ldq + (k ? 0 : 8)), *K = (char *)malloc(s * (size_t)n * ldk + (k ? 0 : 8)), *V = (char *)malloc(s * (size_t)n * ldv);
    char *O = (char *)malloc(s * (size_t)m * ldo);
    size_t got = fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f);
    fclose(f);
    memset(O, 0xFF, s * (size_t)m * ldo); // NaN poison
    csr5::Geometry g{};
    g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
    csr5::DeviceArrays da{};
    da.row_ptr = rp; da.col = col; da.tile_ptr = tp;
    csr5::AttCall c{};
    c.heads = 1; c.k = k; c.d = d;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.O = O; c.ldo = ldo;
    int rc = csr5::launch_mha(g, da, f64 ? CSR5HIP_F64 : CSR5HIP_F32, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(O, s, (size_t)m * ldo, f);
    fclose(f);
    free(rp); free(col); free(tp); free(Q); free(K); free(V); free(O);
    return rc;
}
