// hip_on_host.h -- what a kernel file of probabilisticsemslam_amd/csrc needs to compile for the HOST, line for line: a workgroup is
// block.x std::threads, __syncthreads a std::barrier, the wave operations (ballot, the DPP butterfly, the wave minima) go through
// per-wave barriers with the lane semantics of gfx950.  The workgroups of a launch run one after another; static __shared__ data
// is a static, dynamic LDS (KB_DYNAMIC_LDS) a heap block of exactly the size the launch asks for, so that AddressSanitizer sees any
// access beyond it.  It stands in for kbest_wave.h.  Include it before the kernel files; C++20, -lpthread.
#ifndef HIP_ON_HOST_H
#define HIP_ON_HOST_H
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>
#define KBEST_WAVE_H
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __constant__
#define __launch_bounds__(...)
typedef unsigned long long u64;
typedef unsigned u32;
struct dim3 { int x = 1, y = 1, z = 1; dim3(int a = 1, int b = 1, int c = 1) : x(a), y(b), z(c) {} };
thread_local dim3 threadIdx, blockIdx, gridDim, blockDim;
typedef int hipError_t;
typedef void *hipStream_t;
const int hipSuccess = 0, hipErrorInvalidValue = 1, hipFuncAttributeMaxDynamicSharedMemorySize = 0;
inline int hipGetLastError() { return 0; }
inline int hipGetDevice(int *d) { *d = 0; return 0; }
inline int hipFuncSetAttribute(const void *, int, int) { return 0; }
const int EMU_MAX_WAVES = 16;  // 1 024 threads
static std::barrier<> *wgBar;
static std::barrier<> *waveBar[EMU_MAX_WAVES];
static double xbuf[EMU_MAX_WAVES][64];
static u32 ubuf[EMU_MAX_WAVES][64];
static unsigned char *hostLds;  // the workgroup's dynamic LDS
#define KB_DYNAMIC_LDS(name) unsigned char *name = hostLds
// What a workgroup finds in its fresh block of dynamic LDS (a device does not clear LDS between workgroups): 0 = nothing is written
// (the default: the block is as operator new left it), 1 = every byte 0x00, 2 = every byte 0xFF, 3 = bytes of a generator seeded
// with emuLdsSeed and the workgroup's index.
static int emuLdsFill = 0;
static unsigned long long emuLdsSeed = 0;
inline void emu_fill_bytes(unsigned char *p, size_t n, int fill, unsigned long long seed)
{
    if (fill == 1) memset(p, 0x00, n);
    else if (fill == 2) memset(p, 0xFF, n);
    else if (fill == 3) {
        unsigned long long s = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
        for (size_t i = 0; i < n; i++) {  // splitmix64, one byte of every draw
            s += 0x9E3779B97F4A7C15ull;
            unsigned long long z = s;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            p[i] = (unsigned char)((z ^ (z >> 31)) >> 24);
        }
    }
}
inline void __syncthreads() { wgBar->arrive_and_wait(); }
inline int __popcll(u64 x) { return __builtin_popcountll(x); }
inline int __popc(unsigned x) { return __builtin_popcount(x); }
inline int __ffs(unsigned x) { return __builtin_ffs((int)x); }
inline double __longlong_as_double(long long v)
{
    double d;
    memcpy(&d, &v, 8);
    return d;
}
inline u64 __ballot(bool p)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    ubuf[w][l] = p;
    waveBar[w]->arrive_and_wait();
    u64 r = 0;
    for (int i = 0; i < 64; i++) r |= (u64)(ubuf[w][i] & 1) << i;
    waveBar[w]->arrive_and_wait();
    return r;
}
// ---- the lane-level operations of the k-best kernels (tests/cpp/lane_host.cpp).  One exchange: every lane of the wave publishes a
// value, the wave's barrier, every lane reads the lane it wants.  Two buffers taken in turn: a lane that writes buffer p again has
// passed the barrier of the exchange in between, which every lane reaches only after its read of p -- one barrier per exchange.
static u64 xchgBuf[2][EMU_MAX_WAVES][64];
static thread_local unsigned xchgTurn;
template <class T>
inline T emu_xchg(T x, int src)
{
    static_assert(sizeof(T) <= 8, "one 64-bit word per lane");
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const unsigned p = xchgTurn++ & 1u;
    u64 bits = 0;
    memcpy(&bits, &x, sizeof(T));
    __atomic_store_n(&xchgBuf[p][w][l], bits, __ATOMIC_RELAXED);
    waveBar[w]->arrive_and_wait();
    bits = __atomic_load_n(&xchgBuf[p][w][src & 63], __ATOMIC_RELAXED);
    T r;
    memcpy(&r, &bits, sizeof(T));
    return r;
}
inline int __shfl(int x, int src) { return emu_xchg(x, src & 63); }
inline int __shfl_down(int x, int d) { const int l = threadIdx.x & 63; return emu_xchg(x, l + d < 64 ? l + d : l); }
inline int __shfl_up(int x, int d) { const int l = threadIdx.x & 63; return emu_xchg(x, l - d >= 0 ? l - d : l); }
inline int __builtin_amdgcn_readlane(int x, int l) { return emu_xchg(x, l & 63); }
inline int __builtin_amdgcn_readfirstlane(int x) { return emu_xchg(x, 0); }  // (every lane of the wave is active wherever the kernels call it)
// DPP, every bank enabled: a quad_perm control word (below 0x100: two bits per lane of the quad), row_shr:n (0x111 .. 0x11F),
// row_bcast:15 (0x142) and row_bcast:31 (0x143).  A lane whose row is not in rowMask keeps `old`; a lane whose source lies outside
// its row (row_shr) or does not exist (the broadcasts into rows 0 / 0 and 1) reads 0 with boundCtrl and keeps `old` without.
inline int __builtin_amdgcn_update_dpp(int old, int x, int ctrl, int rowMask, int bankMask, bool boundCtrl)
{
    if (bankMask != 0xF) abort();
    const int l = threadIdx.x & 63, row = l >> 4;
    int src = -1;
    if (ctrl >= 0 && ctrl < 0x100) src = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3);
    else if (ctrl >= 0x111 && ctrl <= 0x11F) src = (l & 15) >= (ctrl & 15) ? l - (ctrl & 15) : -1;
    else if (ctrl == 0x142) src = row >= 1 ? row * 16 - 1 : -1;
    else if (ctrl == 0x143) src = row >= 2 ? 31 : -1;
    else abort();
    const int got = emu_xchg(x, src >= 0 ? src : l);
    if (!((rowMask >> row) & 1)) return old;
    return src >= 0 ? got : (boundCtrl ? 0 : old);
}
inline u32 __builtin_amdgcn_mbcnt_lo(u32 mask, u32 base) { const int l = threadIdx.x & 63; return base + (u32)__builtin_popcount(l >= 32 ? mask : (mask & ((1u << l) - 1u))); }
inline u32 __builtin_amdgcn_mbcnt_hi(u32 mask, u32 base) { const int l = threadIdx.x & 63; return base + (u32)__builtin_popcount(l <= 32 ? 0u : (mask & ((1u << (l - 32)) - 1u))); }
inline bool __builtin_amdgcn_inverse_ballot_w64(u64 mask) { return ((mask >> (threadIdx.x & 63)) & 1ull) != 0ull; }
inline u64 __builtin_amdgcn_read_exec() { return ~0ull; }
#define __builtin_amdgcn_fence(order, scope) __atomic_thread_fence(order)
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __HIP_MEMORY_SCOPE_WORKGROUP 0
#define __hip_atomic_load(ptr, order, scope) __atomic_load_n(ptr, order)
#define __hip_atomic_store(ptr, value, order, scope) __atomic_store_n(ptr, value, order)
#define __hip_atomic_fetch_add(ptr, value, order, scope) __atomic_fetch_add(ptr, value, order)
inline void __builtin_amdgcn_s_sleep(int) { std::this_thread::yield(); }
inline void emu_waitcnt() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }  // s_waitcnt vmcnt(0): this thread's stores are out
inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline unsigned atomicAdd(unsigned *p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
inline int atomicSub(int *p, int v) { return __atomic_fetch_sub(p, v, __ATOMIC_RELAXED); }
inline int atomicOr(int *p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline unsigned long long atomicOr(unsigned long long *p, unsigned long long v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
inline int atomicMin(int *p, int v)
{
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
    return old;
}
template <class T>
inline T emu_atomic_min(T *p, T v)
{
    T old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
    return old;
}
inline unsigned atomicMin(unsigned *p, unsigned v) { return emu_atomic_min(p, v); }
inline unsigned long long atomicMin(unsigned long long *p, unsigned long long v) { return emu_atomic_min(p, v); }
struct alignas(16) double2 { double x, y; };
struct alignas(16) float4 { float x, y, z, w; };
struct alignas(16) int4 { int x, y, z, w; };
struct alignas(16) uint4 { unsigned x, y, z, w; };
struct alignas(4) char4 { signed char x, y, z, w; };
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
inline int __double2hiint(double d) { u64 b; memcpy(&b, &d, 8); return (int)(u32)(b >> 32); }
inline int __double2loint(double d) { u64 b; memcpy(&b, &d, 8); return (int)(u32)b; }
inline double __hiloint2double(int hi, int lo) { const u64 b = ((u64)(u32)hi << 32) | (u32)lo; double d; memcpy(&d, &b, 8); return d; }
inline float __int_as_float(int i) { float f; memcpy(&f, &i, 4); return f; }
inline long long __double_as_longlong(double d) { long long v; memcpy(&v, &d, 8); return v; }
inline float __double2float_ru(double x) { float f = (float)x; return (double)f < x ? nextafterf(f, INFINITY) : f; }   // round up
inline float __double2float_rd(double x) { float f = (float)x; return (double)f > x ? nextafterf(f, -INFINITY) : f; }  // round down
namespace kb {
constexpr int KEY_INF_HI = 0x7ff00000;  // kbest_wave.h's keys
inline void to_key(double x, int &khi, u32 &klo)
{
    const int hi = __double2hiint(x), lo = __double2loint(x);
    const int s = hi >> 31;
    khi = hi ^ (int)((u32)s >> 1);
    klo = (u32)(lo ^ s);
}
inline double from_key(int khi, u32 klo)
{
    const int s = khi >> 31;
    return __hiloint2double(khi ^ (int)((u32)s >> 1), (int)klo ^ s);
}
inline int uni32(int x) { return __builtin_amdgcn_readfirstlane(x); }
inline u64 uni64(u64 x) { return emu_xchg(x, 0); }
inline int sel32(u64 mask, int ifset, int ifclear) { return ((mask >> (threadIdx.x & 63)) & 1ull) ? ifset : ifclear; }
inline double readlane_f64(double x, int l) { return emu_xchg(x, l & 63); }
inline void wave_fence() { waveBar[threadIdx.x >> 6]->arrive_and_wait(); }  // a wave barrier: the lanes are threads here
inline u64 bit64(int i) { return 1ull << (i & 63); }
inline void put_index(int *table, long long i, int value, bool i8)
{
    if (i8) reinterpret_cast<signed char *>(table)[i] = (signed char)value;
    else table[i] = value;
}
inline int wave_min_i32(int x)
{
    int r = x;
    for (int s = 1; s < 64; s <<= 1) {  // butterfly: every lane ends with the minimum of all 64
        const int o = emu_xchg(r, (int)(threadIdx.x & 63) ^ s);
        r = o < r ? o : r;
    }
    return r;
}
inline double d_inf() { return INFINITY; }
inline double min_keep(double a, double b) { return b < a ? b : a; }
inline u32 wave_min_u32(u32 x)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    ubuf[w][l] = x;
    waveBar[w]->arrive_and_wait();
    u32 r = ubuf[w][0];
    for (int i = 1; i < 64; i++) r = ubuf[w][i] < r ? ubuf[w][i] : r;
    waveBar[w]->arrive_and_wait();
    return r;
}
inline double wave_min_f64(double x)  // wave-uniform, as the device's
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    xbuf[w][l] = x;
    waveBar[w]->arrive_and_wait();
    double r = xbuf[w][0];
    for (int i = 1; i < 64; i++) r = min_keep(r, xbuf[w][i]);
    waveBar[w]->arrive_and_wait();
    return r;
}
template <int CTRL, int ROWMASK>
inline double dpp_f64(double x)
{
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, row = l >> 4;
    xbuf[w][l] = x;
    waveBar[w]->arrive_and_wait();
    double r = x;
    if ((ROWMASK >> row) & 1) {
        int src = l;
        if (CTRL < 0x100) src = (l & ~3) | ((CTRL >> (2 * (l & 3))) & 3);  // quad_perm (0xB1: lane ^ 1, 0x4E: lane ^ 2)
        else if (CTRL == 0x141) src = (l & ~7) | (7 - (l & 7));
        else if (CTRL == 0x140) src = (l & ~15) | (15 - (l & 15));
        else if (CTRL == 0x142) src = row * 16 - 1;
        else if (CTRL == 0x143) src = 31;
        else abort();
        r = xbuf[w][src];
    }
    waveBar[w]->arrive_and_wait();
    return r;
}
}
// block.x threads (whole waves) and block.x / 64 wave barriers, whatever the program launches; the workgroups of the launch one
// after another (a two-dimensional grid: x fastest) on the same threads, each with a fresh block of dynamic LDS (the barriers around a workgroup: its static LDS and
// hostLds are the next one's).  lds = 0 is the normal case: only sample_host, lane_host and engine_host launch with dynamic LDS.
template <class K, class... A>
void emu_launch(K kernel, dim3 grid, dim3 block, int lds, A... args)
{
    if (block.x % 64 || block.x > 64 * EMU_MAX_WAVES) abort();
    std::barrier<> wg(block.x);
    wgBar = &wg;
    std::vector<std::unique_ptr<std::barrier<>>> wv;
    for (int w = 0; w < block.x / 64; w++) {
        wv.emplace_back(new std::barrier<>(64));
        waveBar[w] = wv.back().get();
    }
    std::vector<std::thread> th;
    for (int t = 0; t < block.x; t++)
        th.emplace_back([=]() {
            threadIdx = dim3(t);
            gridDim = grid;
            blockDim = block;
            for (int by = 0; by < grid.y; by++)      // (y outer, x inner: piece j of a relay launch finds piece j - 1 finished)
                for (int b = 0; b < grid.x; b++) {
                    blockIdx = dim3(b, by);
                    if (t == 0) {
                        hostLds = new unsigned char[lds];
                        emu_fill_bytes(hostLds, (size_t)lds, emuLdsFill, emuLdsSeed + (unsigned long long)by * (unsigned long long)grid.x + (unsigned long long)b);
                    }
                    wgBar->arrive_and_wait();
                    kernel(args...);
                    wgBar->arrive_and_wait();
                    if (t == 0) delete[] hostLds;
                }
        });
    for (auto &t : th) t.join();
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(kernel, grid, block, lds, __VA_ARGS__)
#endif
