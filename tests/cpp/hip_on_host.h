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
#define __launch_bounds__(x)
typedef unsigned long long u64;
typedef unsigned u32;
struct dim3 { int x = 1, y = 1, z = 1; dim3(int a = 1, int b = 1, int c = 1) : x(a), y(b), z(c) {} };
thread_local dim3 threadIdx, blockIdx, gridDim, blockDim;
typedef int hipError_t;
typedef void *hipStream_t;
const int hipSuccess = 0, hipFuncAttributeMaxDynamicSharedMemorySize = 0;
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
namespace kb {
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
        if (CTRL == 0xB1) src = l ^ 1;
        else if (CTRL == 0x4E) src = l ^ 2;
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
// after another on the same threads, each with a fresh block of dynamic LDS (the barriers around a workgroup: its static LDS and
// hostLds are the next one's).  lds = 0 is the normal case: of the five programs only sample_host launches with dynamic LDS.
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
            for (int b = 0; b < grid.x; b++) {
                blockIdx = dim3(b);
                if (t == 0) hostLds = new unsigned char[lds];
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
