// Stand-alone CPU run of the attention units (csr5_attention*.hip) on the stand-in runtime of fake/hip/hip_runtime.h: the one driver of
// every attention emulation.  It reads a case file written by emulation.py (the layout: DESIGN.md, "The attention emulation's case
// file"), fills ONE csr5::AttBwdCall, dispatches on (variant, mode) to the unit's launcher and writes every output it allocated,
// wanted or not.
//   * Every block is a heap allocation of EXACTLY its declared size (operands and outputs rows * ld elements, B and dB nnz * ldb, a
//     heads * k, dAr m * lddar, the map nnz words, the mask nnz * ldm bytes, the workspace 4 * m * heads elements -- float for the 16-bit
//     kinds), so -fsanitize=address sees any access outside it.
//   * A block the case does not have (has_b, has_a, has_slopes, has_map, has_values = 0; dB of the plain variant; dAr outside the
//     additive ones) is a NULL POINTER in the call, not a spare allocation: a kernel that reads it crashes.
//   * Outputs and the workspace are poisoned with 0xFF before the launch.
// The units are chosen at compile time, -DEMU_<UNIT> per csr5_<unit>.hip (emulation.py build): a program holds exactly the units its
// runner names, and a case for a unit that was left out ends with exit code 2.
#include "csr5_internal.h"
#include "csr5hip_lowp.h"
#include <cstdlib>
#include <vector>

namespace csr5 {
static hipError_t absent(const char *unit)
{
    fprintf(stderr, "attention_driver: built without -DEMU_%s\n", unit);
    exit(2);
}
#define ABSENT_FWD(fn, unit) hipError_t fn(const Geometry &, const DeviceArrays &, int, const AttCall &, hipStream_t) { return absent(unit); }
#define ABSENT_BWD(fn, unit) hipError_t fn(const Geometry &, const DeviceArrays &, int, const AttBwdCall &, hipStream_t) { return absent(unit); }
} // namespace csr5
#ifdef EMU_ATTENTION
#include "csr5_attention.hip"
#else
namespace csr5 { ABSENT_FWD(launch_mha, "ATTENTION") }
#endif
#ifdef EMU_ATTENTION_BWD
#include "csr5_attention_bwd.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_bwd, "ATTENTION_BWD") }
#endif
#ifdef EMU_ATTENTION_BIAS
#include "csr5_attention_bias.hip"
#else
namespace csr5 { ABSENT_FWD(launch_mha_biased, "ATTENTION_BIAS") }
#endif
#ifdef EMU_ATTENTION_BWD_BIAS
#include "csr5_attention_bwd_bias.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_biased_bwd, "ATTENTION_BWD_BIAS") }
#endif
#ifdef EMU_ATTENTION_EDGE
#include "csr5_attention_edge.hip"
#else
namespace csr5 { ABSENT_FWD(launch_mha_edge, "ATTENTION_EDGE") }
#endif
#ifdef EMU_ATTENTION_BWD_EDGE
#include "csr5_attention_bwd_edge.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_edge_bwd, "ATTENTION_BWD_EDGE") }
#endif
#ifdef EMU_ATTENTION_LOWP
#include "csr5_attention_lowp.hip"
#else
namespace csr5 { ABSENT_FWD(launch_mha_lowp, "ATTENTION_LOWP") }
#endif
#ifdef EMU_ATTENTION_BWD_LOWP
#include "csr5_attention_bwd_lowp.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_lowp_bwd, "ATTENTION_BWD_LOWP") }
#endif
#ifdef EMU_ATTENTION_GAT
#include "csr5_attention_gat.hip"
#else
namespace csr5 { ABSENT_FWD(launch_gat, "ATTENTION_GAT") }
#endif
#ifdef EMU_ATTENTION_BWD_GAT
#include "csr5_attention_bwd_gat.hip"
#else
namespace csr5 { ABSENT_BWD(launch_gat_bwd, "ATTENTION_BWD_GAT") }
#endif
#ifdef EMU_ATTENTION_DROP
#include "csr5_attention_drop.hip"
#else
namespace csr5 {
ABSENT_FWD(launch_mha_drop, "ATTENTION_DROP")
hipError_t launch_dropout_mask(int, const AttCall &, unsigned char *, int, hipStream_t) { return absent("ATTENTION_DROP"); }
}
#endif
#ifdef EMU_ATTENTION_BWD_DROP
#include "csr5_attention_bwd_drop.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_drop_bwd, "ATTENTION_BWD_DROP") }
#endif
#ifdef EMU_ATTENTION_DROP_GAT
#include "csr5_attention_drop_gat.hip"
#else
namespace csr5 { ABSENT_FWD(launch_gat_drop, "ATTENTION_DROP_GAT") }
#endif
#ifdef EMU_ATTENTION_BWD_DROP_GAT
#include "csr5_attention_bwd_drop_gat.hip"
#else
namespace csr5 { ABSENT_BWD(launch_gat_drop_bwd, "ATTENTION_BWD_DROP_GAT") }
#endif
#ifdef EMU_ATTENTION_DROP_LOWP
#include "csr5_attention_drop_lowp.hip"
#else
namespace csr5 { ABSENT_FWD(launch_mha_lowp_drop, "ATTENTION_DROP_LOWP") }
#endif
#ifdef EMU_ATTENTION_BWD_DROP_LOWP
#include "csr5_attention_bwd_drop_lowp.hip"
#else
namespace csr5 { ABSENT_BWD(launch_mha_lowp_drop_bwd, "ATTENTION_BWD_DROP_LOWP") }
#endif

// The case file's header: emulation.py's MAGIC, the number of fields, then the fields IN THIS ORDER (emulation.py FIELDS).
constexpr uint32_t MAGIC = 0x35545441; // "ATT5"
enum Variant { PLAIN, BIASED, EDGE, LOWP, GAT, DROP, DROP_GAT, DROP_LOWP, VARIANTS };
enum Mode { FORWARD, BACKWARD, MASK };
struct Header {
    int32_t variant, mode, kind;            // kind: CSR5HIP_F64, CSR5HIP_F32, CSR5HIP_BF16, CSR5HIP_F16
    int32_t m, n, nnz, sigma, p;            // A
    int32_t sigma_t, p_t;                   // A^T (n x m, nnz entries), in the file when mode = BACKWARD
    int32_t k, d, heads, groups;
    int32_t ldq, ldk, ldv, ldo;             // ldo: of O (forward) or of dO (backward)
    int32_t lddq, lddk, lddv, ldb, lddb, lddar, ldm, want; // want: 1 dQ, 2 dK, 4 dV, 8 dB (biased: dS), 16 dAr
    int32_t has_b, has_a, has_slopes, has_values, has_map, head0;
    int32_t offk, offd;                     // the call's pointers start this many columns into the rows (a head's slices, heads = 1)
};
struct Scalars {
    double scale, negative_slope, p;
    uint64_t seed, offset;
};

static std::vector<void *> blocks; // every allocation, freed at the end
static bool short_read = false;
static char *block(size_t bytes)
{
    blocks.push_back(malloc(bytes ? bytes : 1)); // (an empty block keeps a pointer of its own)
    return (char *)blocks.back();
}
static char *from_file(FILE *f, size_t bytes)
{
    char *p = block(bytes);
    short_read |= fread(p, 1, bytes, f) != bytes;
    return p;
}
static char *poisoned(size_t bytes)
{
    return (char *)memset(block(bytes), 0xFF, bytes); // NaN in every element type
}

struct Pattern {
    csr5::Geometry g{};
    csr5::DeviceArrays da{};
    // value_size 0: NO VALUE ARRAY (da.val stays null), so a kernel that reads the handle's values crashes
    void read(FILE *f, int m, int n, int nnz, int sigma, int p, size_t value_size)
    {
        g.m = m; g.n = n; g.nnz = nnz; g.sigma = sigma; g.p = p; g.tile_elems = 64 * sigma;
        da.row_ptr = (int32_t *)from_file(f, 4 * (size_t)(m + 1));
        da.col = (int32_t *)from_file(f, 4 * (size_t)nnz);
        da.tile_ptr = (uint32_t *)from_file(f, 4 * (size_t)(p + 1));
        if (value_size)
            da.val = from_file(f, value_size * (size_t)nnz);
    }
};

static const float *widened(int kind, const void *src, size_t count)
{
    if (!src)
        return nullptr;
    float *out = (float *)block(4 * count);
    for (size_t i = 0; i < count; i++)
        out[i] = kind == CSR5HIP_BF16 ? (float)((const __bf16 *)src)[i] : (float)((const _Float16 *)src)[i];
    return out;
}

struct Block {
    char *p;
    size_t bytes;
};
// The outputs of one launch in file order, poisoned, in elements of s bytes (the workspace: ws), and the wanted ones in the call:
// forward O; backward dQ, dK, dV, dB (not PLAIN), dAr (GAT, DROP_GAT), the workspace (in the call when dK or dV is wanted).
static std::vector<Block> outputs(const Header &h, size_t s, size_t ws, csr5::AttBwdCall &c)
{
    std::vector<Block> o;
    auto out = [&](size_t rows, size_t ld, size_t size) {
        o.push_back({poisoned(size * rows * ld), size * rows * ld});
        return o.back().p;
    };
    if (h.mode == FORWARD) {
        c.O = out(h.m, h.ldo, s) + s * h.offd;
        return o;
    }
    char *dQ = out(h.m, h.lddq, s), *dK = out(h.n, h.lddk, s), *dV = out(h.n, h.lddv, s);
    char *dB = h.variant != PLAIN ? out(h.nnz, h.lddb, s) : nullptr;
    char *dAr = h.variant == GAT || h.variant == DROP_GAT ? out(h.m, h.lddar, s) : nullptr;
    char *work = out(4 * (size_t)h.m, h.heads, ws);
    c.dQ = h.want & 1 ? dQ + s * h.offk : nullptr;
    c.dK = h.want & 2 ? dK + s * h.offk : nullptr;
    c.dV = h.want & 4 ? dV + s * h.offd : nullptr;
    c.dS = h.want & 8 ? dB : nullptr;
    c.dAr = h.want & 16 ? dAr : nullptr;
    c.work = h.want & 6 ? work : nullptr;
    return o;
}

static int launch(int variant, int mode, const Pattern &A, int type, const csr5::AttBwdCall &c)
{
    using namespace csr5;
    using Forward = hipError_t(const Geometry &, const DeviceArrays &, int, const AttCall &, hipStream_t);
    using Backward = hipError_t(const Geometry &, const DeviceArrays &, int, const AttBwdCall &, hipStream_t);
    static Forward *const forward[VARIANTS] = {launch_mha, launch_mha_biased, launch_mha_edge, launch_mha_lowp, launch_gat, launch_mha_drop,
                                               launch_gat_drop, launch_mha_lowp_drop};
    static Backward *const backward[VARIANTS] = {launch_mha_bwd, launch_mha_biased_bwd, launch_mha_edge_bwd, launch_mha_lowp_bwd,
                                                 launch_gat_bwd, launch_mha_drop_bwd, launch_gat_drop_bwd, launch_mha_lowp_drop_bwd};
    return mode == FORWARD ? forward[variant](A.g, A.da, type, c, nullptr) : backward[variant](A.g, A.da, type, c, nullptr);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    uint32_t lead[2];
    Header h;
    Scalars x;
    if (!f || fread(lead, 4, 2, f) != 2 || lead[0] != MAGIC || lead[1] != sizeof(Header) / 4) {
        fprintf(stderr, "attention_driver: %s is not a case of this driver's layout (%zu fields)\n", argv[1], sizeof(Header) / 4);
        return 2;
    }
    if (fread(&h, sizeof h, 1, f) != 1 || fread(&x, sizeof x, 1, f) != 1) return 2;
    if (h.variant < 0 || h.variant >= VARIANTS || h.mode < FORWARD || h.mode > MASK || h.kind < CSR5HIP_F64 || h.kind > CSR5HIP_F16 ||
        (h.variant == LOWP || h.variant == DROP_LOWP) != (h.kind >= CSR5HIP_BF16) || (h.mode == MASK && h.variant != DROP && h.variant != DROP_GAT))
        return 2;
    const size_t s = h.kind == CSR5HIP_F64 ? 8 : h.kind == CSR5HIP_F32 ? 4 : 2, ws = s == 2 ? 4 : s;
    const size_t m = h.m, n = h.n, nnz = h.nnz;
    Pattern A, At;
    A.read(f, h.m, h.n, h.nnz, h.sigma, h.p, h.has_values ? s : 0);
    if (h.mode == BACKWARD)
        At.read(f, h.n, h.m, h.nnz, h.sigma_t, h.p_t, h.has_values ? s : 0);
    const uint32_t *map = h.has_map ? (const uint32_t *)from_file(f, 4 * nnz) : nullptr;
    csr5::AttBwdCall c{};
    c.heads = h.heads; c.groups = h.groups; c.k = h.k; c.d = h.d;
    c.scale = x.scale; c.negative_slope = x.negative_slope; c.p = x.p; c.seed = x.seed; c.offset = x.offset; c.head0 = h.head0;
    c.a = h.has_a ? from_file(f, s * (size_t)h.heads * h.k) : nullptr;
    c.slopes = h.has_slopes ? from_file(f, s * (size_t)h.heads) : nullptr;
    c.B = h.has_b ? from_file(f, s * nnz * h.ldb) : nullptr;
    c.ldb = h.ldb; c.ldq = h.ldq; c.ldk = h.ldk; c.ldv = h.ldv; c.ldo = c.lddo = h.ldo;
    c.lddq = h.lddq; c.lddk = h.lddk; c.lddv = h.lddv; c.ldds = h.lddb; c.lddar = h.lddar;
    const char *Q = nullptr, *K = nullptr, *V = nullptr, *dO = nullptr;
    if (h.mode != MASK) { // the pointers of the call start offk / offd columns into the rows
        Q = from_file(f, s * m * h.ldq); K = from_file(f, s * n * h.ldk); V = from_file(f, s * n * h.ldv);
        c.Q = Q + s * h.offk; c.K = K + s * h.offk; c.V = V + s * h.offd;
    }
    if (h.mode == BACKWARD) {
        dO = from_file(f, s * m * h.ldo);
        c.dO = dO + s * h.offd;
        if (h.want & 6) { // the column side's companion
            c.gt = &At.g; c.dt = &At.da; c.map = map;
        }
    }
    const bool complete = !short_read && fgetc(f) == EOF;
    fclose(f);
    if (!complete) {
        fprintf(stderr, "attention_driver: %s does not hold exactly the blocks its header declares\n", argv[1]);
        return 2;
    }
    std::vector<Block> written;
    int rc;
    if (h.mode == MASK) {
        written.push_back({poisoned(nnz * h.ldm), nnz * h.ldm});
        rc = csr5::launch_dropout_mask(h.nnz, c, (unsigned char *)written[0].p, h.ldm, nullptr);
    } else {
        written = outputs(h, s, ws, c);
        rc = launch(h.variant, h.mode, A, h.kind, c);
    }
    if ((h.variant == LOWP || h.variant == DROP_LOWP) && !rc) { // the same case through the float edge launcher (DROP_LOWP: the float
                                                                // dropped one) on operands widened here, element by element
        c.B = widened(h.kind, c.B, nnz * h.ldb);
        c.Q = widened(h.kind, Q, m * h.ldq) + h.offk; c.K = widened(h.kind, K, n * h.ldk) + h.offk;
        c.V = widened(h.kind, V, n * h.ldv) + h.offd;
        if (dO)
            c.dO = widened(h.kind, dO, m * h.ldo) + h.offd;
        for (const Block &b : outputs(h, 4, 4, c))
            written.push_back(b);
        rc = launch(h.variant == LOWP ? EDGE : DROP, h.mode, A, CSR5HIP_F32, c);
    }
    f = fopen(argv[2], "wb");
    for (const Block &b : written)
        fwrite(b.p, 1, b.bytes, f);
    fclose(f);
    for (void *p : blocks)
        free(p);
    return rc;
}
