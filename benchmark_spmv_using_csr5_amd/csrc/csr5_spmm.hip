// csr5_spmm.hip -- CSR5 SpMM for gfx950 (wave64): Y = A * X for k dense vectors in one pass over the matrix per column block.
//
// X is n x k and Y is m x k, both row-major with leading dimensions ldx / ldy.  One wavefront walks one tile of the plain
// (parent) tile structure exactly as the two-pass SpMV does (csr5_spmv.hip k_spmv<.., FUSED=false> + k_calibrate<.., false>),
// but every element gathers the KB contiguous values of row col of X (KB = 1, 2, 4, 8: a compile-time column block) and
// every running sum is KB sums.  Per column the arithmetic is the SpMV's, operation for operation: the lane-local
// fused-multiply-add walk over the bit flags, the DPP segmented scan of csr5_wave.h, the carries added in tile order by
// sum_run's association, the CSR tail summed through LDS.  So column c of Y is bit-identical to a two-pass spmv() with
// x = X[:, c].  k > 8 runs as ceil(k / 8) passes; a remainder block uses the next KB up with the extra columns masked.
//
// Bytes per pass: the matrix streams once (4 + s per non-zero, s = sizeof value) plus tile_desc and the carries; X is
// gathered KB values per element (one 16-byte load per 16 bytes when X's address and ldx allow, else element loads).
// Registers: sigma * KB gathered values cannot all be in flight (sigma 16 x KB 8 fp64 = 256 VGPRs), so a lane's elements go
// in groups of SPMM_GROUP_VALUES / KB, and the next group's gathers are issued before the current group is consumed.
#include "csr5_carry.h"

// Contraction of a separate multiply and add into one FMA would change the association the SpMV uses: every FMA here is
// written out (fma_vt), every other product stays a rounded product.
#pragma clang fp contract(off)

namespace csr5 {

constexpr int SPMM_GROUP_VALUES = 16; // gathered values of one group of elements (per lane): x2 for the group in flight
constexpr int SPMM_MAX_KB = 8;        // widest column block: k > 8 runs as ceil(k / 8) passes

// KB contiguous values of one row of X (or Y) at p.  VEC: whole-block vector accesses (the block is full and p, ld allow it);
// else element accesses of the first kc values.
template <typename VT, int KB, bool VEC>
__device__ __forceinline__ void load_block(const VT *__restrict__ p, VT (&o)[KB], int kc)
{
    constexpr int BYTES = KB * (int)sizeof(VT);
    if constexpr (VEC && BYTES >= 16) {
        constexpr int PER = 16 / (int)sizeof(VT);
#pragma unroll
        for (int q = 0; q < BYTES / 16; q++) {
            const uint4 w = reinterpret_cast<const uint4 *>(p)[q];
            if constexpr (sizeof(VT) == 8) {
                o[q * PER] = __builtin_bit_cast(double, (unsigned long long)w.y << 32 | w.x);
                o[q * PER + 1] = __builtin_bit_cast(double, (unsigned long long)w.w << 32 | w.z);
            } else {
                o[q * PER] = __builtin_bit_cast(float, w.x);
                o[q * PER + 1] = __builtin_bit_cast(float, w.y);
                o[q * PER + 2] = __builtin_bit_cast(float, w.z);
                o[q * PER + 3] = __builtin_bit_cast(float, w.w);
            }
        }
    } else if constexpr (VEC && BYTES == 8 && sizeof(VT) == 4) { // fp32, KB = 2
        const uint2 w = *reinterpret_cast<const uint2 *>(p);
        o[0] = __builtin_bit_cast(VT, w.x);
        o[1] = __builtin_bit_cast(VT, w.y);
    } else {
#pragma unroll
        for (int j = 0; j < KB; j++)
            o[j] = j < kc ? p[j] : (VT)0;
    }
}
template <typename VT, int KB, bool VEC>
__device__ __forceinline__ void store_block(VT *__restrict__ p, const VT (&v)[KB], int kc)
{
    constexpr int BYTES = KB * (int)sizeof(VT);
    if constexpr (VEC && BYTES >= 16) {
        constexpr int PER = 16 / (int)sizeof(VT);
#pragma unroll
        for (int q = 0; q < BYTES / 16; q++) {
            uint4 w;
            if constexpr (sizeof(VT) == 8) {
                const unsigned long long a = __builtin_bit_cast(unsigned long long, v[q * PER]);
                const unsigned long long b = __builtin_bit_cast(unsigned long long, v[q * PER + 1]);
                w = make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32));
            } else {
                w = make_uint4(__builtin_bit_cast(unsigned, v[q * PER]), __builtin_bit_cast(unsigned, v[q * PER + 1]),
                               __builtin_bit_cast(unsigned, v[q * PER + 2]), __builtin_bit_cast(unsigned, v[q * PER + 3]));
            }
            reinterpret_cast<uint4 *>(p)[q] = w;
        }
    } else if constexpr (VEC && BYTES == 8 && sizeof(VT) == 4) {
        *reinterpret_cast<uint2 *>(p) = make_uint2(__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]));
    } else {
#pragma unroll
        for (int j = 0; j < KB; j++)
            if (j < kc)
                p[j] = v[j];
    }
}

// ---- CSR tail: rows tail_start .. m-1, as tail_rows (csr5_carry.h), one column after the other through the same LDS buffer ----
template <typename VT, int SIGMA, int KB>
__device__ __forceinline__ void spmm_tail(const Geometry &g, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                          const VT *__restrict__ val, const VT *__restrict__ X, int ldx, VT *__restrict__ Y, int ldy,
                                          VT *__restrict__ cal, int kc, int tail_block, VT *sprod)
{
    const int tid = threadIdx.x;
    const int lane = tid & (OMEGA - 1);
    const int first_tail = (g.p - 1) * g.tile_elems;
    const int E = g.nnz - first_tail;
    constexpr int PER = ((SIGMA > 0 ? OMEGA * SIGMA : TAIL_MAX) + BLOCK - 1) / BLOCK;
    int32_t c[PER];
    VT v[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int e = tid + k * BLOCK;
        const int idx = first_tail + (e < E ? e : 0);
        c[k] = col[idx];
        v[k] = val[idx];
    }
    const int r = g.tail_start + tail_block * BLOCK + tid;
    const bool valid = r < g.m;
    int a = 0, b = 0;
    if (valid) {
        a = row_ptr[r];
        b = row_ptr[r + 1];
    }
    a = (r == g.tail_start ? first_tail : a) - first_tail;
    b -= first_tail;
    const bool longrow = valid && (b - a) > 32;
    for (int j = 0; j < kc; j++) {
        VT xv[PER];
#pragma unroll
        for (int k = 0; k < PER; k++)
            xv[k] = X[(size_t)(uint32_t)c[k] * ldx + j];
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int e = tid + k * BLOCK;
            if (e < E)
                sprod[e] = v[k] * xv[k];
        }
        __syncthreads();
        VT sum = 0;
        if (valid && !longrow)
            for (int k = a; k < b; k++)
                sum += sprod[k];
        unsigned long long todo = __ballot(longrow);
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int aa = __shfl(a, src, OMEGA);
            const int bb = __shfl(b, src, OMEGA);
            VT s = 0;
            for (int k = aa + lane; k < bb; k += OMEGA)
                s += sprod[k];
            s = wave_sum(s);
            if (lane == src)
                sum = s;
        }
        if (valid) {
            if (r == g.tail_start)
                cal[(size_t)(g.p - 1) * KB + j] = sum; // the first tail row may have begun before the tail: a carry
            else
                Y[(size_t)r * ldy + j] = sum;
        }
        __syncthreads(); // (the buffer is reused by the next column)
    }
}

// ---- tiles 0..p-2: one tile per wavefront, KB columns ----------------------------------------------------------------------
// SIGMA > 0: compile-time sigma (column / value words and the flag walk unrolled); SIGMA == 0: run-time sigma, same arithmetic.
template <typename VT, int SIGMA, int KB, bool VEC>
__device__ __forceinline__ void spmm_tile(const Geometry &g, const int t, const int lane, const int32_t *__restrict__ col,
                                          const VT *__restrict__ val, const VT *__restrict__ X, const int ldx,
                                          const uint32_t *__restrict__ tile_ptr, const uint32_t *__restrict__ tile_desc,
                                          const int32_t *__restrict__ offset_ptr, const int32_t *__restrict__ offset,
                                          VT *__restrict__ cal, VT *__restrict__ Y, const int ldy, const int kc)
{
    const int sigma = SIGMA > 0 ? SIGMA : g.sigma;
    const int bit_y = SIGMA > 0 ? bit_y_of(SIGMA > 0 ? SIGMA : 1) : g.bit_y;
    const int bit_all = bit_y + BIT_SS;
    const int num_packet = SIGMA > 0 ? num_packet_of(SIGMA > 0 ? SIGMA : 1) : g.num_packet;
    const int T = OMEGA * sigma;
    const size_t base = (size_t)t * T + lane;
    const int32_t *ct = col + base;
    const VT *vt = val + base;
    const uint32_t *d = tile_desc + (size_t)t * OMEGA * num_packet;
    int vz; // opaque per-lane zero: the tile_ptr pair rides the vector-memory round trip of the tile loads (see csr5_spmv.hip)
    asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
    const uint32_t tp0 = tile_ptr[t + vz];
    const uint32_t tp1 = tile_ptr[t + 1 + vz];
    constexpr int NREG = SIGMA > 0 ? SIGMA : 1;
    int32_t c[NREG];
    VT mv[NREG];
    if constexpr (SIGMA > 0) {
#pragma unroll
        for (int i = 0; i < SIGMA; i++)
            c[i] = ct[i * OMEGA];
    }
    const uint32_t w0 = d[lane];
    const uint32_t w1 = num_packet > 1 ? d[OMEGA + lane] : 0u;
    if constexpr (SIGMA > 0) {
#pragma unroll
        for (int i = 0; i < SIGMA; i++)
            mv[i] = vt[i * OMEGA];
    }
    auto xrow = [&](int32_t cw) -> const VT * { return X + (size_t)(uint32_t)cw * ldx; };

    // groups of G elements; two groups of gathers in flight at most
    constexpr int G0 = SPMM_GROUP_VALUES / KB;
    constexpr int G = SIGMA > 0 ? (G0 < SIGMA ? G0 : SIGMA) : 1;
    constexpr int NG = SIGMA > 0 ? (SIGMA + G - 1) / G : 1;
    VT xg[2][G][KB];
    auto issue = [&](int grp) {
#pragma unroll
        for (int e = 0; e < G; e++) {
            const int i = grp * G + e;
            if (i < NREG)
                load_block<VT, KB, VEC>(xrow(c[i]), xg[grp & 1][e], kc);
        }
    };
    if constexpr (SIGMA > 0) {
        issue(0);
        __builtin_amdgcn_sched_barrier(0);
    }

    uint32_t flags = w0 << bit_all; // element i -> bit 31-i
    if (num_packet > 1)
        flags |= w1 >> (32 - bit_all);
    const uint32_t rs_raw = __builtin_amdgcn_readfirstlane(tp0);
    const uint32_t row_stop = __builtin_amdgcn_readfirstlane(tp1) & ROW_MASK;
    // fast track (the whole tile inside one row): csr5_spmv.hip sums every element onto 0 with FMAs and adds the lanes with
    // wave_sum.  With no flags the walk below does the former; only element 0's first operation differs.
    const bool fast = rs_raw == row_stop;
    if (fast)
        flags = 0;
    int y_off = (int)(w0 >> (32 - bit_y));
    const bool f0 = (flags >> 31) | (lane == 0);
    const bool present = f0 | ((flags & 0x7FFFFFFFu) != 0);
    const bool empty_rows = (bool)(rs_raw >> 31);
    const int row_start = (int)(rs_raw & ROW_MASK);
    VT *y_local = Y + (size_t)(row_start + 1) * ldy;
    const int32_t *off_local = empty_rows && !fast ? offset + offset_ptr[t] : nullptr;
    auto put = [&](int idx, const VT (&s)[KB]) {
        store_block<VT, KB, VEC>(y_local + (size_t)(empty_rows ? off_local[idx] : idx) * ldy, s, kc);
    };

    bool direct = f0 && lane != 0;
    VT sum[KB], first_sum[KB];
#pragma unroll
    for (int j = 0; j < KB; j++)
        first_sum[j] = 0;
    // element i of the lane with its gathered block xr
    auto step = [&](int i, VT m, const VT (&xr)[KB]) {
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < KB; j++)
                sum[j] = fast ? fma_vt(m, xr[j], (VT)0) : m * xr[j];
            return;
        }
        if ((flags >> (31 - i)) & 1u) {
            if (direct)
                put(y_off, sum);
            else {
#pragma unroll
                for (int j = 0; j < KB; j++)
                    first_sum[j] = sum[j];
            }
            y_off += direct;
            direct = true;
#pragma unroll
            for (int j = 0; j < KB; j++)
                sum[j] = 0;
        }
#pragma unroll
        for (int j = 0; j < KB; j++)
            sum[j] = fma_vt(m, xr[j], sum[j]);
    };
    if constexpr (SIGMA > 0) {
#pragma unroll
        for (int grp = 0; grp < NG; grp++) {
            if (grp + 1 < NG)
                issue(grp + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < G; e++) {
                const int i = grp * G + e;
                if (i < SIGMA)
                    step(i, mv[i], xg[grp & 1][e]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        for (int i = 0; i < sigma; i++) {
            const int32_t ci = ct[i * OMEGA];
            const VT m = vt[i * OMEGA];
            VT xr[KB];
            load_block<VT, KB, VEC>(xrow(ci), xr, kc);
            step(i, m, xr);
        }
    }

    if (fast) {
#pragma unroll
        for (int j = 0; j < KB; j++)
            sum[j] = wave_sum(sum[j]);
        if (lane == 0)
            store_block<VT, KB, true>(cal + (size_t)t * KB, sum, KB);
        return;
    }
    if (!direct) {
#pragma unroll
        for (int j = 0; j < KB; j++)
            first_sum[j] = sum[j];
    }

    // cross-lane step of csr5_spmv.hip, once per column: S[l] = R[l+1], R[j] = lead[j] + (present[j] ? 0 : R[j+1])
    VT R[KB];
#pragma unroll
    for (int j = 0; j < KB; j++)
        R[j] = f0 ? (VT)0 : first_sum[j];
    const unsigned long long pmask = __ballot(present);
    const unsigned long long z1 = ~pmask;
    if (z1) {
        const unsigned long long ahead = pmask >> lane;
        const int dist = ahead ? __builtin_ctzll(ahead) : OMEGA - 1 - lane;
#pragma unroll
        for (int j = 0; j < KB; j++) {
            const VT up = dpp_move<DPP_ROW_SHL1>(R[j]);
            R[j] += dist >= 1 ? up : (VT)0;
        }
        const unsigned long long z2 = z1 & (z1 >> 1);
        if (z2) {
#pragma unroll
            for (int j = 0; j < KB; j++) {
                const VT up = dpp_move<DPP_ROW_SHL2>(R[j]);
                R[j] += dist >= 2 ? up : (VT)0;
            }
            const unsigned long long z4 = z2 & (z2 >> 2);
            if (z4) {
#pragma unroll
                for (int j = 0; j < KB; j++) {
                    const VT up = dpp_move<DPP_ROW_SHL4>(R[j]);
                    R[j] += dist >= 4 ? up : (VT)0;
                }
                if (z4 & (z4 >> 4)) {
#pragma unroll
                    for (int j = 0; j < KB; j++) {
                        const VT up = dpp_move<DPP_ROW_SHL8>(R[j]);
                        R[j] += dist >= 8 ? up : (VT)0;
                    }
                }
            }
        }
        const int reach = lane + dist;
#pragma unroll
        for (int edge = 48; edge >= 16; edge -= 16) {
            if (!((pmask >> (edge - 1)) & 1ull)) {
                const bool take = (lane >> 4) == (edge >> 4) - 1 && reach >= edge;
#pragma unroll
                for (int j = 0; j < KB; j++) {
                    const VT carry_in = bcast_lane(R[j], edge);
                    R[j] += take ? carry_in : (VT)0;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KB; j++) {
        const VT S = lane_above(R[j]);
        if (present)
            sum[j] += S;
    }
    if (direct)
        put(y_off, sum);
    if (lane == 0)
        store_block<VT, KB, true>(cal + (size_t)t * KB, direct ? first_sum : sum, KB);
}

template <typename VT, int SIGMA, int KB, bool VEC>
__global__ void __launch_bounds__(BLOCK)
k_spmm(Geometry g, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col, const VT *__restrict__ val,
       const VT *__restrict__ X, int ldx, const uint32_t *__restrict__ tile_ptr, const uint32_t *__restrict__ tile_desc,
       const int32_t *__restrict__ offset_ptr, const int32_t *__restrict__ offset, VT *__restrict__ cal, VT *__restrict__ Y,
       int ldy, int kc, int tile_blocks, int xcd_remap)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int blk = blockIdx.x;
    if (blk >= tile_blocks) {
        spmm_tail<VT, SIGMA, KB>(g, row_ptr, col, val, X, ldx, Y, ldy, cal, kc, blk - tile_blocks, reinterpret_cast<VT *>(smem));
        return;
    }
    if (xcd_remap) { // every XCD one contiguous range of tiles (csr5_spmv.hip k_spmv)
        const int q = tile_blocks / NUM_XCD, rem = tile_blocks % NUM_XCD;
        const int xcd = blk % NUM_XCD;
        blk = xcd * q + (xcd < rem ? xcd : rem) + blk / NUM_XCD;
    }
    const int lane = threadIdx.x & (OMEGA - 1);
    const int t = __builtin_amdgcn_readfirstlane(blk * WAVES_PER_BLOCK + (int)(threadIdx.x >> 6));
    if (t >= g.p - 1)
        return;
    spmm_tile<VT, SIGMA, KB, VEC>(g, t, lane, col, val, X, ldx, tile_ptr, tile_desc, offset_ptr, offset, cal, Y, ldy, kc);
}

// ---- carries: k_calibrate<VT, false> over the column block ------------------------------------------------------------------
// One thread per run head; the first carry of a row that begins exactly on a tile boundary stores, otherwise the closing
// partial that k_spmm stored into Y comes first; then the tiles' leading partials in tile order (sum_run's association; runs
// longer than RUN_SERIAL_MAX tiles are summed by the whole wavefront, lane-strided, then wave_sum).
template <typename VT, int KB>
__global__ void __launch_bounds__(BLOCK)
k_spmm_calibrate(Geometry g, const uint32_t *__restrict__ tile_ptr, const uint4 *__restrict__ meta, const VT *__restrict__ cal,
                 VT *__restrict__ Y, int ldy, int kc)
{
    const int lane = threadIdx.x & (OMEGA - 1);
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    bool head = false;
    int len = 0;
    bool has_first = false;
    int r = 0;
    if (t < g.p) {
        const uint4 mt = meta[t];
        head = (int)mt.y == t;
        r = (int)(tile_ptr[t] & ROW_MASK);
        if ((mt.x >> 28) & 1u) { // short-spill head (fused-mode classification): one carry onto Y[r]
            len = 1;
            has_first = true;
        } else {
            has_first = (mt.x >> 27) & 1u;
            len = (int)(mt.x & 0x00FFFFFFu) - (has_first ? 1 : 0);
        }
        head = head && r < g.m && len > 0;
    }
    if (head && len <= RUN_SERIAL_MAX) {
        VT *yr = Y + (size_t)r * ldy;
        const VT *cr = cal + (size_t)t * KB;
        VT total[KB], part[KB];
        load_block<VT, KB, true>(cr, part, KB);
        if (has_first) {
            VT first[KB];
            load_block<VT, KB, false>(yr, first, kc);
#pragma unroll
            for (int j = 0; j < KB; j++)
                total[j] = first[j] + part[j];
        } else {
#pragma unroll
            for (int j = 0; j < KB; j++)
                total[j] = part[j];
        }
        for (int k = 1; k < len; k++) {
            load_block<VT, KB, true>(cr + (size_t)k * KB, part, KB);
#pragma unroll
            for (int j = 0; j < KB; j++)
                total[j] += part[j];
        }
        store_block<VT, KB, false>(yr, total, kc);
    }
    unsigned long long todo = __ballot(head && len > RUN_SERIAL_MAX);
    while (todo) {
        const int leader = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int slot = __shfl(t, leader, OMEGA);
        const int ln = __shfl(len, leader, OMEGA);
        const bool hf = __shfl((int)has_first, leader, OMEGA);
        const int row = __shfl(r, leader, OMEGA);
        VT *yr = Y + (size_t)row * ldy;
        for (int j = 0; j < kc; j++) {
            VT part = 0;
#pragma unroll 4
            for (int k = lane; k < ln; k += OMEGA)
                part += cal[(size_t)(slot + k) * KB + j];
            part = wave_sum(part);
            if (lane == leader)
                yr[j] = hf ? yr[j] + part : part;
        }
    }
}

// CSR5HIP_OPT_ZERO_EMPTY_ROWS: columns 0..kc-1 of every row (the kernels then overwrite every row that owns a non-zero)
template <typename VT>
__global__ void __launch_bounds__(256) k_spmm_zero(int m, int k, VT *__restrict__ Y, int ldy)
{
    const size_t total = (size_t)m * k;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
        Y[(i / k) * ldy + i % k] = 0;
}

// ---- dispatch ----------------------------------------------------------------------------------------------------------------
template <typename VT, int SIGMA, int KB, bool VEC>
static hipError_t spmm_block(const Geometry &g, const DeviceArrays &d, const VT *X, int ldx, VT *Y, int ldy, int kc, VT *cal,
                             int xcd_remap, hipStream_t s)
{
    const int tile_blocks = g.p > 1 ? (g.p - 1 + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK : 0;
    const int tail_rows_n = g.m - g.tail_start;
    const int tail_blocks = tail_rows_n > 0 ? (tail_rows_n + BLOCK - 1) / BLOCK : 0;
    if (tile_blocks + tail_blocks == 0)
        return hipSuccess;
    const size_t lds = (size_t)g.tile_elems * sizeof(VT); // tail product buffer (tail workgroups)
    hipLaunchKernelGGL((k_spmm<VT, SIGMA, KB, VEC>), dim3(tile_blocks + tail_blocks), dim3(BLOCK), lds, s, g, d.row_ptr, d.col,
                       (const VT *)d.val, X, ldx, d.tile_ptr, d.tile_desc, d.offset_ptr, d.offset, cal, Y, ldy, kc, tile_blocks,
                       xcd_remap);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL((k_spmm_calibrate<VT, KB>), dim3((g.p + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, g, d.tile_ptr,
                       reinterpret_cast<const uint4 *>(d.carry_meta), (const VT *)cal, Y, ldy, kc);
    return hipGetLastError();
}

template <typename VT, int SIGMA>
static hipError_t spmm_kb_dispatch(const Geometry &g, const DeviceArrays &d, const VT *X, int ldx, VT *Y, int ldy, int kc, VT *cal,
                                   int xcd_remap, hipStream_t s)
{
    const int KB = spmm_block_width(kc); // (the next width up of 1, 2, 4, 8)
    // whole-block vector accesses: a full block whose rows start on the vector width in X and in Y
    const size_t width = (size_t)KB * sizeof(VT) < 16 ? (size_t)KB * sizeof(VT) : 16;
    const bool vec = kc == KB && width >= 8 && reinterpret_cast<uintptr_t>(X) % width == 0 &&
                     reinterpret_cast<uintptr_t>(Y) % width == 0 && ((size_t)ldx * sizeof(VT)) % width == 0 &&
                     ((size_t)ldy * sizeof(VT)) % width == 0;
    switch (KB) {
    case 1: return spmm_block<VT, SIGMA, 1, false>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
    case 2:
        return vec ? spmm_block<VT, SIGMA, 2, true>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s)
                   : spmm_block<VT, SIGMA, 2, false>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
    case 4:
        return vec ? spmm_block<VT, SIGMA, 4, true>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s)
                   : spmm_block<VT, SIGMA, 4, false>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
    default:
        return vec ? spmm_block<VT, SIGMA, 8, true>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s)
                   : spmm_block<VT, SIGMA, 8, false>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
    }
}

// compile-time sigma for every value the auto rule returns (fp64 6..16, fp32 8..16) plus 4, 24 and 32; run-time sigma otherwise
template <typename VT>
static hipError_t spmm_sigma_dispatch(const Geometry &g, const DeviceArrays &d, const VT *X, int ldx, VT *Y, int ldy, int kc, VT *cal,
                                      int xcd_remap, hipStream_t s)
{
#define CSR5_SPMM_CASE(S) \
    case S: return spmm_kb_dispatch<VT, S>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
    if constexpr (sizeof(VT) == 8) {
        switch (g.sigma) {
            CSR5_SPMM_CASE(4) CSR5_SPMM_CASE(6) CSR5_SPMM_CASE(7) CSR5_SPMM_CASE(8) CSR5_SPMM_CASE(9) CSR5_SPMM_CASE(10)
            CSR5_SPMM_CASE(11) CSR5_SPMM_CASE(12) CSR5_SPMM_CASE(13) CSR5_SPMM_CASE(14) CSR5_SPMM_CASE(15) CSR5_SPMM_CASE(16)
            CSR5_SPMM_CASE(24) CSR5_SPMM_CASE(32)
        default: break;
        }
    } else {
        switch (g.sigma) {
            CSR5_SPMM_CASE(4) CSR5_SPMM_CASE(8) CSR5_SPMM_CASE(9) CSR5_SPMM_CASE(10) CSR5_SPMM_CASE(11) CSR5_SPMM_CASE(12)
            CSR5_SPMM_CASE(13) CSR5_SPMM_CASE(14) CSR5_SPMM_CASE(15) CSR5_SPMM_CASE(16) CSR5_SPMM_CASE(24) CSR5_SPMM_CASE(32)
        default: break;
        }
    }
#undef CSR5_SPMM_CASE
    return spmm_kb_dispatch<VT, 0>(g, d, X, ldx, Y, ldy, kc, cal, xcd_remap, s);
}

template <typename VT>
static hipError_t spmm_typed(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, void *Y, int ldy, void *work,
                             int zero_empty, int xcd_remap, hipStream_t s)
{
    if (zero_empty && g.m > 0) {
        const size_t total = (size_t)g.m * k;
        size_t blocks = (total + 255) / 256;
        blocks = blocks < 4096 ? blocks : 4096;
        hipLaunchKernelGGL((k_spmm_zero<VT>), dim3((unsigned)blocks), dim3(256), 0, s, g.m, k, (VT *)Y, ldy);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    if (g.p <= 0)
        return hipSuccess;
    for (int c0 = 0; c0 < k; c0 += SPMM_MAX_KB) {
        const int kc = k - c0 < SPMM_MAX_KB ? k - c0 : SPMM_MAX_KB;
        const hipError_t e = spmm_sigma_dispatch<VT>(g, d, (const VT *)X + c0, ldx, (VT *)Y + c0, ldy, kc, (VT *)work, xcd_remap, s);
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

// The product build compiles this file twice (-DCSR5_SPMM_ONLY_F64 / -DCSR5_SPMM_ONLY_F32), as csr5_spmv.hip.
#if !defined(CSR5_SPMM_ONLY_F32)
hipError_t launch_spmm_f64(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, void *Y, int ldy, void *work,
                           int zero_empty, int xcd_remap, hipStream_t s)
{
    return spmm_typed<double>(g, d, X, ldx, k, Y, ldy, work, zero_empty, xcd_remap, s);
}
#endif
#if !defined(CSR5_SPMM_ONLY_F64)
hipError_t launch_spmm_f32(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, void *Y, int ldy, void *work,
                           int zero_empty, int xcd_remap, hipStream_t s)
{
    return spmm_typed<float>(g, d, X, ldx, k, Y, ldy, work, zero_empty, xcd_remap, s);
}
#endif

#if !defined(CSR5_SPMM_ONLY_F32)
hipError_t launch_spmm_f32(const Geometry &g, const DeviceArrays &d, const void *X, int ldx, int k, void *Y, int ldy, void *work,
                           int zero_empty, int xcd_remap, hipStream_t s);

hipError_t launch_spmm(const Geometry &g, const DeviceArrays &d, int value_type, const void *X, int ldx, int k, void *Y, int ldy,
                       void *work, int zero_empty, int xcd_remap, hipStream_t s)
{
    return value_type == CSR5HIP_F64 ? launch_spmm_f64(g, d, X, ldx, k, Y, ldy, work, zero_empty, xcd_remap, s)
                                     : launch_spmm_f32(g, d, X, ldx, k, Y, ldy, work, zero_empty, xcd_remap, s);
}
#endif

} // namespace csr5
