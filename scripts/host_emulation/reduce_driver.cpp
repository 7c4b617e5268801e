// Stand-alone CPU run of csr5_reduce.hip on the stand-in runtime of fake/hip/hip_runtime.h: the driver of run_spmm_reduce.py.  It reads
// one case file, calls the unit's launcher for the case's mode and writes every output it allocated.
//   * Every block is a heap allocation of EXACTLY its declared size (operands and outputs rows * ld elements, the map and dval nnz), so
//     -fsanitize=address sees any access outside it.
//   * A block the case does not have (the values when unweighted, arg when not wanted) is a NULL POINTER: a kernel that reads it crashes.
//   * Outputs are poisoned before the launch: 0xFF bytes (NaN) for values, 0x7B bytes for arg (-1 is a legal arg).
// The case file: MAGIC, the number of header fields, the header (struct Header, run_spmm_reduce.py FIELDS), then the blocks in the
// order main() reads them.
#include "csr5_internal.h"
#include <cstdlib>
#include <vector>

#include "csr5_reduce.hip"

constexpr uint32_t MAGIC = 0x35444552; // "RED5"
enum Mode { FORWARD, DVAL, DX };
struct Header {
    int32_t mode, kind, op, weighted, has_arg;
    int32_t m, nnz, sigma, p, k; // the pattern walked: A's (FORWARD, DVAL) or the companion's (DX: m = A's columns)
    int32_t xrows, grows;        // rows of X (A's columns); rows of dY and arg (A's rows)
    int32_t ldx, ldg, ldarg, ldo; // ldg: of dY; ldo: of Y (FORWARD) or dX (DX)
};

static std::vector<void *> blocks;
static bool short_read = false;
static char *block(size_t bytes)
{
    blocks.push_back(malloc(bytes ? bytes : 1));
    return (char *)blocks.back();
}
static char *from_file(FILE *f, size_t bytes)
{
    char *p = block(bytes);
    short_read |= fread(p, 1, bytes, f) != bytes;
    return p;
}
static char *poisoned(size_t bytes, int byte)
{
    return (char *)memset(block(bytes), byte, bytes);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t lead[2];
    Header h;
    if (!f || fread(lead, 4, 2, f) != 2 || lead[0] != MAGIC || lead[1] != sizeof(Header) / 4 || fread(&h, sizeof h, 1, f) != 1) {
        fprintf(stderr, "reduce_driver: %s is not a case of this driver's layout\n", argv[1]);
        return 2;
    }
    if (h.mode < FORWARD || h.mode > DX || (h.kind != CSR5HIP_F64 && h.kind != CSR5HIP_F32)) return 2;
    const size_t s = h.kind == CSR5HIP_F64 ? 8 : 4, m = h.m, nnz = h.nnz, k = h.k;
    csr5::Geometry g{};
    csr5::DeviceArrays d{};
    g.m = h.m; g.nnz = h.nnz; g.sigma = h.sigma; g.p = h.p; g.tile_elems = 64 * h.sigma;
    d.row_ptr = (int32_t *)from_file(f, 4 * (m + 1));
    d.col = (int32_t *)from_file(f, 4 * nnz);
    d.tile_ptr = (uint32_t *)from_file(f, 4 * (size_t)(h.p + 1));
    if (h.weighted && h.mode != DVAL)
        d.val = from_file(f, s * nnz);
    const uint32_t *map = h.mode == DX ? (const uint32_t *)from_file(f, 4 * nnz) : nullptr;
    const char *X = h.mode != DX ? from_file(f, s * (size_t)h.xrows * h.ldx) : nullptr;
    const char *dY = h.mode != FORWARD ? from_file(f, s * (size_t)h.grows * h.ldg) : nullptr;
    const int32_t *arg_in = h.mode != FORWARD ? (const int32_t *)from_file(f, 4 * (size_t)h.grows * h.ldarg) : nullptr;
    const bool complete = !short_read && fgetc(f) == EOF;
    fclose(f);
    if (!complete) {
        fprintf(stderr, "reduce_driver: %s does not hold exactly the blocks its header declares\n", argv[1]);
        return 2;
    }
    struct Out { char *p; size_t bytes; };
    std::vector<Out> written;
    int rc;
    if (h.mode == FORWARD) {
        written.push_back({poisoned(s * m * h.ldo, 0xFF), s * m * h.ldo});
        if (h.has_arg)
            written.push_back({poisoned(4 * m * h.ldarg, 0x7B), 4 * m * h.ldarg});
        rc = csr5::launch_spmm_reduce(g, d, h.kind, h.op, h.weighted, X, h.ldx, h.k, written[0].p, h.ldo,
                                      h.has_arg ? (int32_t *)written[1].p : nullptr, h.ldarg, nullptr);
    } else if (h.mode == DVAL) {
        written.push_back({poisoned(s * nnz, 0xFF), s * nnz});
        rc = csr5::launch_spmm_reduce_dval(g, d, h.kind, X, h.ldx, h.k, dY, h.ldg, arg_in, h.ldarg, written[0].p, nullptr);
    } else {
        written.push_back({poisoned(s * m * h.ldo, 0xFF), s * m * h.ldo});
        rc = csr5::launch_spmm_reduce_dx(g, d, map, h.kind, h.weighted, h.k, dY, h.ldg, arg_in, h.ldarg, written[0].p, h.ldo, nullptr);
    }
    (void)k;
    f = fopen(argv[2], "wb");
    for (const Out &o : written)
        fwrite(o.p, 1, o.bytes, f);
    fclose(f);
    for (void *p : blocks)
        free(p);
    return rc;
}
