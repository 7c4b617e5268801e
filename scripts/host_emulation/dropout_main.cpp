// Stand-alone CPU run of the dropped attention entries (csr5_attention_drop.hip, csr5_attention_drop_gat.hip and their backwards) on the
// stand-in runtime of fake/hip/hip_runtime.h: reads a case file written by run_dropout.py (header; the scale, the negative slope and p;
// seed and offset; row_ptr, tile-ordered columns and tile_ptr of the matrix and of its transpose; the source map (position in A^T's
// CSR -> position in A's CSR); a; B; packed Q, K, V and, backward, dO) and writes, forward (mode 0), O; backward (mode 1), dQ, dK,
// dV, dB, dAr; mode 2, the mask of launch_dropout_mask, nnz rows of ldb bytes.  family 0: launch_mha_drop / launch_mha_drop_bwd (a and
// dAr unused); family 1: launch_gat_drop / launch_gat_drop_bwd.  THE PATTERNS HAVE NO VALUE ARRAYS (null pointers).  Every operand, a,
// B, dB, dAr, the mask, the workspace and the map is a heap block of EXACTLY its declared size: an index beyond one is an access
// -fsanitize=address reports.
#include "csr5_attention_drop.hip"
#include "csr5_attention_drop_gat.hip"
#include "csr5_attention_bwd_drop.hip"
#include "csr5_attention_bwd_drop_gat.hip"
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
        da.row_ptr = rp; da.col = col; da.tile_ptr = tp; da.val = nullptr;
        return fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f);
    }
    void release() { free(rp); free(col); free(tp); }
};
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[28];
    double sc[3];
    unsigned long long so[2];
    if (!f || fread(h, 4, 28, f) != 28 || fread(sc, 8, 3, f) != 3 || fread(so, 8, 2, f) != 2) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], sigma_t = h[5], p_t = h[6], k = h[7], d = h[8];
    const int ldq = h[9], ldk = h[10], ldv = h[11], lddo = h[12], lddq = h[13], lddk = h[14], lddv = h[15], f64 = h[16], want = h[17];
    const int heads = h[18], groups = h[19], has_b = h[20], ldb = h[21], lddb = h[22], has_a = h[23], lddar = h[24], mode = h[25];
    const int family = h[26], head0 = h[27];
    const size_t s = f64 ? 8 : 4;
    Pattern A, At;
    size_t got = A.read(f, m, n, nnz, sigma, p) + At.read(f, n, m, nnz, sigma_t, p_t);
    auto block = [&](size_t rows, size_t ld) { return (char *)malloc(s * rows * ld + (rows * ld ? 0 : 8)); };
    const size_t wn = 4 * (size_t)m * heads;
    uint32_t *map = (uint32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    char *a = block(1, (size_t)heads * k), *B = block(nnz, ldb);
    char *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *dO = block(m, lddo); // (mode 0: dO's block is O, lddo its ldo)
    char *dQ = block(m, lddq), *dK = block(n, lddk), *dV = block(n, lddv), *work = block(1, wn), *dB = block(nnz, lddb);
    char *dAr = block(m, lddar);
    got += fread(map, 4, nnz, f) + fread(a, s, (size_t)heads * k, f) + fread(B, s, (size_t)nnz * ldb, f);
    got += fread(Q, s, (size_t)m * ldq, f) + fread(K, s, (size_t)n * ldk, f) + fread(V, s, (size_t)n * ldv, f);
    if (mode)
        got += fread(dO, s, (size_t)m * lddo, f);
    else
        memset(dO, 0xFF, s * (size_t)m * lddo);
    fclose(f);
    memset(dQ, 0xFF, s * (size_t)m * lddq); // NaN poison
    memset(dK, 0xFF, s * (size_t)n * lddk);
    memset(dV, 0xFF, s * (size_t)n * lddv);
    memset(dB, 0xFF, s * (size_t)nnz * lddb);
    memset(dAr, 0xFF, s * (size_t)m * lddar);
    memset(work, 0xFF, s * wn);
    const bool column = want & 6;
    csr5::AttBwdCall c{};
    c.heads = heads; c.groups = groups; c.k = k; c.d = d; c.scale = sc[0]; c.negative_slope = sc[1]; c.a = has_a ? a : nullptr;
    c.B = has_b ? B : nullptr; c.ldb = ldb;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv;
    c.p = sc[2]; c.seed = so[0]; c.offset = so[1]; c.head0 = head0;
    const int vt = f64 ? CSR5HIP_F64 : CSR5HIP_F32;
    unsigned char *mask = (unsigned char *)malloc((size_t)nnz * ldb + (nnz ? 0 : 8));
    memset(mask, 0xAB, (size_t)nnz * ldb);
    int rc;
    if (mode == 2) {
        rc = csr5::launch_dropout_mask(nnz, c, mask, ldb, nullptr);
    } else if (mode) {
        c.dO = dO; c.lddo = lddo;
        c.dQ = want & 1 ? dQ : nullptr; c.dK = want & 2 ? dK : nullptr; c.dV = want & 4 ? dV : nullptr;
        c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
        c.work = column ? work : nullptr; c.dS = want & 8 ? dB : nullptr; c.ldds = lddb;
        c.dAr = want & 16 ? dAr : nullptr; c.lddar = lddar;
        c.gt = column ? &At.g : nullptr; c.dt = column ? &At.da : nullptr; c.map = column ? map : nullptr;
        rc = family ? csr5::launch_gat_drop_bwd(A.g, A.da, vt, c, nullptr) : csr5::launch_mha_drop_bwd(A.g, A.da, vt, c, nullptr);
    } else {
        c.O = dO; c.ldo = lddo;
        rc = family ? csr5::launch_gat_drop(A.g, A.da, vt, c, nullptr) : csr5::launch_mha_drop(A.g, A.da, vt, c, nullptr);
    }
    f = fopen(argv[2], "wb");
    if (mode == 2) {
        fwrite(mask, 1, (size_t)nnz * ldb, f);
    } else if (mode) {
        fwrite(dQ, s, (size_t)m * lddq, f);
        fwrite(dK, s, (size_t)n * lddk, f);
        fwrite(dV, s, (size_t)n * lddv, f);
        fwrite(dB, s, (size_t)nnz * lddb, f);
        fwrite(dAr, s, (size_t)m * lddar, f);
    } else {
        fwrite(dO, s, (size_t)m * lddo, f);
    }
    fclose(f);
    A.release(); At.release();
    free(map); free(a); free(B); free(Q); free(K); free(V); free(dO); free(dQ); free(dK); free(dV); free(work); free(dB); free(dAr); free(mask);
    (void)got;
    return rc;
}
