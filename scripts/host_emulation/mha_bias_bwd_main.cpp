// Stand-alone CPU run of csr5_attention_bwd_bias.hip's entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file
// written by run_mha_bias.py (header; the scale; row_ptr, tile-ordered columns, tile_ptr and tile-ordered values of the matrix and
// of its transpose; slopes; packed Q, K, V, dO), writes dQ, dK, dV, dS.  launch_mha_biased_bwd with `heads` heads, `groups` head
// groups (0: the rule) and a workspace of exactly 4 m heads values; dS is a block of exactly nnz ldds values.  Every array is a
// heap block of its exact size.
#include "csr5_attention_bwd_bias.hip"
#include <cstdlib>
struct Pattern {
    int32_t *rp, *col;
    uint32_t *tp;
    char *val;
    csr5::Geometry g{};
    csr5::DeviceArrays da{};
    size_t read(FILE *f, size_t s, int m, int n, int nnz, int sigma, int p)
    {
        rp = (int32_t *)malloc(4 * (size_t)(m + 1));
        col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
        tp = (uint32_t *)malloc(4 * (size_t)(p + 1));
        val = (char *)malloc(s * (size_t)(nnz ? nnz : 1));
        g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
        da.row_ptr = rp; da.col = col; da.tile_ptr = tp; da.val = val;
        return fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f) + fread(val, s, nnz, f);
    }
    void release() { free(rp); free(col); free(tp); free(val); }
};
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[22];
    double scale;
    if (!f || fread(h, 4, 22, f) != 22 || fread(&scale, 8, 1, f) != 1) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], sigma_t = h[5], p_t = h[6], k = h[7], d = h[8];
    const int ldq = h[9], ldk = h[10], ldv = h[11], lddo = h[12], lddq = h[13], lddk = h[14], lddv = h[15], f64 = h[16], want = h[17];
    const int heads = h[18], groups = h[19], has_slopes = h[20], ldds = h[21];
    const size_t s = f64 ? 8 : 4;
    Pattern A, At;
    size_t got = A.read(f, s, m, n, nnz, sigma, p) + At.read(f, s, n, m, nnz, sigma_t, p_t);
    auto block = [&](int rows, int ld) { return (char *)malloc(s * (size_t)rows * ld + (ld ? 0 : 8)); };
    const size_t wn = 4 * (size_t)m * heads;
    char *slopes = (char *)malloc(s * (size_t)(heads ? heads : 1));
    char *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *dO = block(m, lddo);
    char *dQ = block(m, lddq), *dK = block(n, lddk), *dV = block(n, lddv), *work = (char *)malloc(s * wn + 8), *dS = block(nnz, ldds);
    got += fread(slopes, s, heads, f);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f) + fread(dO, s, (size_t)m * lddo, f);
    fclose(f);
    memset(dQ, 0xFF, s * (size_t)m * lddq); // NaN poison
    memset(dK, 0xFF, s * (size_t)n * lddk);
    memset(dV, 0xFF, s * (size_t)n * lddv);
    memset(dS, 0xFF, s * (size_t)nnz * ldds);
    memset(work, 0xFF, s * wn);
    const bool column = want & 6;
    csr5::AttBwdCall c{};
    c.heads = heads; c.groups = groups; c.k = k; c.d = d; c.scale = scale; c.slopes = has_slopes ? slopes : nullptr;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.dO = dO; c.lddo = lddo;
    c.dQ = want & 1 ? dQ : nullptr; c.dK = want & 2 ? dK : nullptr; c.dV = want & 4 ? dV : nullptr;
    c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
    c.work = column ? work : nullptr; c.dS = want & 8 ? dS : nullptr; c.ldds = ldds;
    c.gt = column ? &At.g : nullptr; c.dt = column ? &At.da : nullptr;
    const int rc = csr5::launch_mha_biased_bwd(A.g, A.da, f64 ? CSR5HIP_F64 : CSR5HIP_F32, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(dQ, s, (size_t)m * lddq, f);
    fwrite(dK, s, (size_t)n * lddk, f);
    fwrite(dV, s, (size_t)n * lddv, f);
    fwrite(dS, s, (size_t)nnz * ldds, f);
    fclose(f);
    A.release(); At.release();
    free(slopes); free(Q); free(K); free(V); free(dO); free(dQ); free(dK); free(dV); free(work); free(dS);
    return rc;
}
