// Stand-alone CPU run of csr5_attention_bwd_lowp.hip's entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file
// written by run_mha_lowp_backward.py (header; the scale; row_ptr, tile-ordered columns and tile_ptr of the matrix and of its
// transpose; the source map; then B and packed Q, K, V, dO as 16-BIT WORDS of the operand type), runs launch_mha_lowp_bwd with `heads`
// heads and `groups` head groups (0: the rule) and writes the words of dQ, dK, dV, dB and the float workspace.  Every operand, every
// output, B, dB, the workspace (exactly 4 m heads floats) and the map (exactly nnz words) is a heap block of EXACTLY its declared
// size, so -fsanitize=address sees an index computed in 4-byte units, a 16-byte load past a row's end or a wrong rank.  THE PATTERNS
// HAVE NO VALUE ARRAYS (null pointers).
// Then the same case goes through csr5_attention_bwd_edge.hip's float launcher on operands widened here, element by element, and its
// float outputs and workspace are written after the first: the script rounds them itself and compares the words.
#include "csr5_attention_bwd_edge.hip"
#include "csr5_attention_bwd_lowp.hip"
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

template <typename ST>
static float *widened(const void *src, size_t count)
{
    float *out = (float *)malloc(4 * (count ? count : 1));
    for (size_t i = 0; i < count; i++)
        out[i] = (float)((const ST *)src)[i];
    return out;
}

static char *poisoned(size_t bytes)
{
    char *p = (char *)malloc(bytes ? bytes : 8);
    memset(p, 0xFF, bytes); // NaN poison in every type
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[23];
    double scale;
    if (!f || fread(h, 4, 23, f) != 23 || fread(&scale, 8, 1, f) != 1) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], sigma_t = h[5], p_t = h[6], k = h[7], d = h[8];
    const int ldq = h[9], ldk = h[10], ldv = h[11], lddo = h[12], lddq = h[13], lddk = h[14], lddv = h[15], bf16 = h[16], want = h[17];
    const int heads = h[18], groups = h[19], has_b = h[20], ldb = h[21], lddb = h[22];
    Pattern A, At;
    size_t got = A.read(f, m, n, nnz, sigma, p) + At.read(f, n, m, nnz, sigma_t, p_t);
    auto count = [](int rows, int ld) { return (size_t)rows * ld; };
    auto block = [&](int rows, int ld) { return (char *)malloc(2 * count(rows, ld) + (count(rows, ld) ? 0 : 8)); };
    const size_t wn = 4 * (size_t)m * heads;
    uint32_t *map = (uint32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    char *B = block(nnz, ldb), *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *dO = block(m, lddo);
    got += fread(map, 4, nnz, f) + fread(B, 2, count(nnz, ldb), f);
    got += fread(Q, 2, count(m, ldq), f) + fread(K, 2, count(n, ldk), f) + fread(V, 2, count(n, ldv), f) + fread(dO, 2, count(m, lddo), f);
    fclose(f);
    if (got != (size_t)(m + 1) + (n + 1) + 2 * (size_t)nnz + (p + 1) + (p_t + 1) + nnz + count(nnz, ldb) + count(m, ldq) + count(n, ldk) +
                   count(n, ldv) + count(m, lddo))
        return 2;
    const size_t sizes[4] = {count(m, lddq), count(n, lddk), count(n, lddv), count(nnz, lddb)};
    char *out16[4], *out32[4];
    for (int i = 0; i < 4; i++) {
        out16[i] = poisoned(2 * sizes[i]);
        out32[i] = poisoned(4 * sizes[i]);
    }
    char *work16 = poisoned(4 * wn), *work32 = poisoned(4 * wn); // (both FLOAT: work16 is the 16-bit call's)
    const bool column = want & 6;
    csr5::AttBwdCall c{};
    c.heads = heads; c.groups = groups; c.k = k; c.d = d; c.scale = scale; c.B = has_b ? B : nullptr; c.ldb = ldb;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.dO = dO; c.lddo = lddo;
    c.dQ = want & 1 ? out16[0] : nullptr; c.dK = want & 2 ? out16[1] : nullptr; c.dV = want & 4 ? out16[2] : nullptr;
    c.lddq = lddq; c.lddk = lddk; c.lddv = lddv;
    c.work = column ? work16 : nullptr; c.dS = want & 8 ? out16[3] : nullptr; c.ldds = lddb;
    c.gt = column ? &At.g : nullptr; c.dt = column ? &At.da : nullptr; c.map = column ? map : nullptr;
    int rc = csr5::launch_mha_lowp_bwd(A.g, A.da, bf16 ? CSR5HIP_BF16 : CSR5HIP_F16, c, nullptr);
    float *B32 = bf16 ? widened<__bf16>(B, count(nnz, ldb)) : widened<_Float16>(B, count(nnz, ldb));
    float *Q32 = bf16 ? widened<__bf16>(Q, count(m, ldq)) : widened<_Float16>(Q, count(m, ldq));
    float *K32 = bf16 ? widened<__bf16>(K, count(n, ldk)) : widened<_Float16>(K, count(n, ldk));
    float *V32 = bf16 ? widened<__bf16>(V, count(n, ldv)) : widened<_Float16>(V, count(n, ldv));
    float *dO32 = bf16 ? widened<__bf16>(dO, count(m, lddo)) : widened<_Float16>(dO, count(m, lddo));
    c.B = has_b ? B32 : nullptr; c.Q = Q32; c.K = K32; c.V = V32; c.dO = dO32;
    c.dQ = want & 1 ? out32[0] : nullptr; c.dK = want & 2 ? out32[1] : nullptr; c.dV = want & 4 ? out32[2] : nullptr;
    c.work = column ? work32 : nullptr; c.dS = want & 8 ? out32[3] : nullptr;
    if (!rc)
        rc = csr5::launch_mha_edge_bwd(A.g, A.da, CSR5HIP_F32, c, nullptr);
    f = fopen(argv[2], "wb");
    for (int i = 0; i < 4; i++)
        fwrite(out16[i], 2, sizes[i], f);
    fwrite(work16, 4, wn, f);
    for (int i = 0; i < 4; i++)
        fwrite(out32[i], 4, sizes[i], f);
    fwrite(work32, 4, wn, f);
    fclose(f);
    A.release(); At.release();
    free(map); free(B); free(Q); free(K); free(V); free(dO); free(work16); free(work32);
    free(B32); free(Q32); free(K32); free(V32); free(dO32);
    for (int i = 0; i < 4; i++) {
        free(out16[i]);
        free(out32[i]);
    }
    return rc;
}
