// Stand-alone CPU run of csr5_attention_edge.hip's entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file written
// by run_mha_edge_bias.py (header, the scale, row_ptr, tile-ordered columns, tile_ptr, B, packed Q, K, V), writes O.
// launch_mha_edge with `heads` heads and `groups` head groups (0: the rule); B is passed only when the header says so.  THE
// PATTERN HAS NO VALUE ARRAY (a null pointer): a read of the handle's values would fault.  B is a heap block of EXACTLY nnz ldb
// values, like every other array of its exact size, so -fsanitize=address sees any access outside it.
#include "csr5_attention_edge.hip"
#include <cstdlib>
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[16];
    double scale;
    if (!f || fread(h, 4, 16, f) != 16 || fread(&scale, 8, 1, f) != 1) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], k = h[5], d = h[6], ldq = h[7], ldk = h[8], ldv = h[9], ldo = h[10], f64 = h[11];
    const int heads = h[12], groups = h[13], has_b = h[14], ldb = h[15];
    const size_t s = f64 ? 8 : 4;
    int32_t *rp = (int32_t *)malloc(4 * (size_t)(m + 1)), *col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    uint32_t *tp = (uint32_t *)malloc(4 * (size_t)(p + 1));
    auto block = [&](int rows, int ld) { return (char *)malloc(s * (size_t)rows * ld + ((size_t)rows * ld ? 0 : 8)); };
    char *B = block(nnz, ldb), *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *O = block(m, ldo);
    size_t got = fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f) + fread(B, s, (size_t)nnz * ldb, f);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f);
    fclose(f);
    memset(O, 0xFF, s * (size_t)m * ldo); // NaN poison
    csr5::Geometry g{};
    g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
    csr5::DeviceArrays da{};
    da.row_ptr = rp; da.col = col; da.tile_ptr = tp; da.val = nullptr;
    csr5::AttCall c{};
    c.heads = heads; c.groups = groups; c.k = k; c.d = d; c.scale = scale; c.B = has_b ? B : nullptr; c.ldb = ldb;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.O = O; c.ldo = ldo;
    const int rc = csr5::launch_mha_edge(g, da, f64 ? CSR5HIP_F64 : CSR5HIP_F32, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(O, s, (size_t)m * ldo, f);
    fclose(f);
    free(rp); free(col); free(tp); free(B); free(Q); free(K); free(V); free(O);
    return rc;
}
