// Host stand-in for <hip/hip_runtime.h>, for running a row-wise kernel of csrc/ on the CPU (scripts/host_emulation/run_attention.py):
// a workgroup is 256 std::threads, __shared__ is a static, and every cross-lane operation (__shfl, __ballot, DPP moves, readlane) is
// an exchange through a per-wavefront barrier, so it must be reached by all 64 lanes of a wavefront -- as on the GPU.  Workgroups
// run one after the other.  Only what csr5_wave.h and csr5_attention.hip use is here.
#pragma once
#include <atomic>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
typedef int hipError_t;
constexpr int hipSuccess = 0;
typedef void *hipStream_t;
inline hipError_t hipGetLastError() { return 0; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { unsigned x, y, z, w; };
struct Idx { unsigned x, y, z; };
inline thread_local Idx threadIdx, blockIdx;
struct EmuWave { std::barrier<> bar{64}; uint64_t x[64]; };
inline EmuWave emu_waves[4];
inline std::barrier<> emu_block{256};
inline void emu_gather(uint64_t v, uint64_t *out)
{
    EmuWave &w = emu_waves[threadIdx.x >> 6];
    w.x[threadIdx.x & 63] = v;
    w.bar.arrive_and_wait();
    memcpy(out, w.x, sizeof(w.x));
    w.bar.arrive_and_wait();
}
template <typename T> inline uint64_t emu_bits(T v) { uint64_t b = 0; memcpy(&b, &v, sizeof(T)); return b; }
template <typename T> inline T emu_val(uint64_t b) { T v; memcpy(&v, &b, sizeof(T)); return v; }
template <typename T> inline T __shfl(T v, int src, int = 64) { uint64_t a[64]; emu_gather(emu_bits(v), a); return emu_val<T>(a[src & 63]); }
template <typename T> inline T __shfl_xor(T v, int m, int = 64) { return __shfl(v, (int)(threadIdx.x & 63) ^ m); }
inline unsigned long long __ballot(int p) { uint64_t a[64]; emu_gather(p ? 1 : 0, a); unsigned long long r = 0; for (int i = 0; i < 64; i++) r |= (unsigned long long)(a[i] & 1) << i; return r; }
inline int __any(int p) { return __ballot(p) != 0; }
inline void __syncthreads() { emu_block.arrive_and_wait(); }
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline int emu_readlane(int v, int src) { return __shfl(v, src); }
inline int emu_readfirstlane(int v) { return __shfl(v, 0); }
inline int emu_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound)
{
    uint64_t a[64];
    emu_gather((uint32_t)src, a);
    const int l = threadIdx.x & 63, r = l >> 4, p = l & 15;
    int from = -1;
    if (ctrl < 0x100) from = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);
    else if (ctrl >= 0x101 && ctrl <= 0x10F) { int n = ctrl & 15; from = p + n <= 15 ? l + n : -1; }
    else if (ctrl >= 0x111 && ctrl <= 0x11F) { int n = ctrl & 15; from = p >= n ? l - n : -1; }
    else if (ctrl == 0x140) from = (l & ~15) | (15 - p);
    else if (ctrl == 0x141) from = (l & ~7) | (7 - (l & 7));
    else if (ctrl == 0x142) from = r >= 1 ? 16 * r - 1 : -1;
    else if (ctrl == 0x143) from = r >= 2 ? 31 : -1;
    else { fprintf(stderr, "emu: dpp ctrl %x\n", ctrl); abort(); }
    if (!((row_mask >> r) & 1) || !((bank_mask >> ((l >> 2) & 3)) & 1)) return old;
    if (from < 0) return bound ? 0 : old;
    return (int)(uint32_t)a[from];
}
#define __builtin_amdgcn_update_dpp emu_dpp
#define __builtin_amdgcn_readlane emu_readlane
#define __builtin_amdgcn_readfirstlane emu_readfirstlane
#define __builtin_amdgcn_fence(a, b) ((void)0)
#define __builtin_amdgcn_wave_barrier() emu_waves[threadIdx.x >> 6].bar.arrive_and_wait()
template <typename K, typename... Args>
inline void emu_launch(K kernel, dim3 grid, dim3 block, Args... args)
{
    if (block.x != 256) { fprintf(stderr, "emu: block %u\n", block.x); abort(); }
    for (unsigned by = 0; by < grid.y; by++)
        for (unsigned b = 0; b < grid.x; b++) {
            std::vector<std::thread> ts;
            for (unsigned t = 0; t < 256; t++)
                ts.emplace_back([=] { threadIdx = {t, 0, 0}; blockIdx = {b, by, 0}; kernel(args...); });
            for (auto &t : ts) t.join();
        }
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
