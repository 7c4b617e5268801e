// Stand-alone CPU run of csr5_attention_lowp.hip's entry on the stand-in runtime of fake/hip/hip_runtime.h: reads a case file written
// by run_mha_lowp.py (header, the scale, row_ptr, tile-ordered columns, tile_ptr, then B and packed Q, K, V as 16-BIT WORDS of the
// operand type), runs launch_mha_lowp with `heads` heads and `groups` head groups (0: the rule) and writes O's words.  Q, K, V, B and
// O are heap blocks of EXACTLY rows * ld 2-byte elements, so -fsanitize=address sees an index computed in 4-byte units or a 16-byte
// load past a row's end.  THE PATTERN HAS NO VALUE ARRAY (a null pointer).
// Then the same case goes through csr5_attention_edge.hip's float launcher on operands widened here, element by element, and that O
// (float) is written after the first: the script rounds it itself and compares the words.
#include "csr5_attention_edge.hip"
#include "csr5_attention_lowp.hip"
#include <cstdlib>

template <typename ST>
static float *widened(const void *src, size_t count)
{
    float *out = (float *)malloc(4 * (count ? count : 1));
    for (size_t i = 0; i < count; i++)
        out[i] = (float)((const ST *)src)[i];
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    int h[16];
    double scale;
    if (!f || fread(h, 4, 16, f) != 16 || fread(&scale, 8, 1, f) != 1) return 2;
    const int m = h[0], n = h[1], nnz = h[2], sigma = h[3], p = h[4], k = h[5], d = h[6], ldq = h[7], ldk = h[8], ldv = h[9], ldo = h[10], bf16 = h[11];
    const int heads = h[12], groups = h[13], has_b = h[14], ldb = h[15];
    int32_t *rp = (int32_t *)malloc(4 * (size_t)(m + 1)), *col = (int32_t *)malloc(4 * (size_t)(nnz ? nnz : 1));
    uint32_t *tp = (uint32_t *)malloc(4 * (size_t)(p + 1));
    auto count = [](int rows, int ld) { return (size_t)rows * ld; };
    auto block = [&](int rows, int ld) { return (char *)malloc(2 * count(rows, ld) + (count(rows, ld) ? 0 : 8)); };
    char *B = block(nnz, ldb), *Q = block(m, ldq), *K = block(n, ldk), *V = block(n, ldv), *O = block(m, ldo);
    size_t got = fread(rp, 4, m + 1, f) + fread(col, 4, nnz, f) + fread(tp, 4, p + 1, f) + fread(B, 2, count(nnz, ldb), f);
    got += fread(Q, 2, count(m, ldq), f) + fread(K, 2, count(n, ldk), f) + fread(V, 2, count(n, ldv), f);
    fclose(f);
    if (got != (size_t)(m + 1) + nnz + (p + 1) + count(nnz, ldb) + count(m, ldq) + count(n, ldk) + count(n, ldv)) return 2;
    memset(O, 0xFF, 2 * count(m, ldo)); // NaN poison
    csr5::Geometry g{};
    g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
    csr5::DeviceArrays da{};
    da.row_ptr = rp; da.col = col; da.tile_ptr = tp; da.val = nullptr;
    csr5::AttCall c{};
    c.heads = heads; c.groups = groups; c.k = k; c.d = d; c.scale = scale; c.B = has_b ? B : nullptr; c.ldb = ldb;
    c.Q = Q; c.ldq = ldq; c.K = K; c.ldk = ldk; c.V = V; c.ldv = ldv; c.O = O; c.ldo = ldo;
    int rc = csr5::launch_mha_lowp(g, da, bf16 ? CSR5HIP_BF16 : CSR5HIP_F16, c, nullptr);
    float *B32 = bf16 ? widened<__bf16>(B, count(nnz, ldb)) : widened<_Float16>(B, count(nnz, ldb));
    float *Q32 = bf16 ? widened<__bf16>(Q, count(m, ldq)) : widened<_Float16>(Q, count(m, ldq));
    float *K32 = bf16 ? widened<__bf16>(K, count(n, ldk)) : widened<_Float16>(K, count(n, ldk));
    float *V32 = bf16 ? widened<__bf16>(V, count(n, ldv)) : widened<_Float16>(V, count(n, ldv));
    float *O32 = (float *)malloc(4 * (count(m, ldo) ? count(m, ldo) : 1));
    memset(O32, 0xFF, 4 * count(m, ldo));
    c.B = has_b ? B32 : nullptr; c.Q = Q32; c.K = K32; c.V = V32; c.O = O32;
    if (!rc)
        rc = csr5::launch_mha_edge(g, da, CSR5HIP_F32, c, nullptr);
    f = fopen(argv[2], "wb");
    fwrite(O, 2, count(m, ldo), f);
    fwrite(O32, 4, count(m, ldo), f);
    fclose(f);
    free(rp); free(col); free(tp); free(B); free(Q); free(K); free(V); free(O);
    free(B32); free(Q32); free(K32); free(V32); free(O32);
    return rc;
}
