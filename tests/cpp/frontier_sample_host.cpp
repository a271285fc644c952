// kbest_frontier_sample.hip compiled for the HOST, line for line, as tests/cpp/frontier_host.cpp compiles kbest_frontier.hip: a
// workgroup is 256 std::threads, __syncthreads a std::barrier, the wave operations go through per-wave barriers with the lane
// semantics of gfx950.  Built with -fsanitize=address,undefined and run on exact-size heap buffers, it checks what a GPU run cannot
// show without risk: that neither the sweep nor the walk reads or writes beyond the slot, the plan, the row keys or the outputs.
// tests/test_frontier_sample_cpu.py builds and runs it.
// usage: frontier_sample_host IN OUT [slotDoubles [grid]]
//   IN: int n, nSample; u64 seed; u32 sampleBase, pad; per cluster int m, nL; u64 frameKey; the (nL + m) * m doubles of its
//       sub-block; the nL + m int32 keys of its rows.
//   OUT: per cluster int info, width; double logZ; nSample * m int32 (assignLocal, -5: untouched); nSample doubles (logTerm, -5.0)
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
thread_local dim3 threadIdx, blockIdx, gridDim;
typedef int hipError_t;
typedef void *hipStream_t;
const int hipSuccess = 0;
inline int hipGetLastError() { return 0; }
static std::barrier<> *wgBar;
static std::barrier<> *waveBar[4];
static double xbuf[4][64];
static u32 ubuf[4][64];
inline void __syncthreads() { wgBar->arrive_and_wait(); }
inline int __popcll(u64 x) { return __builtin_popcountll(x); }
inline int __ffs(unsigned x) { return __builtin_ffs((int)x); }
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
template <class K, class... A>
void emu_launch(K kernel, dim3 grid, dim3 block, A... args)
{
    for (int b = 0; b < grid.x; b++) {
        std::barrier<> wg(block.x), w0(64), w1(64), w2(64), w3(64);
        wgBar = &wg; waveBar[0] = &w0; waveBar[1] = &w1; waveBar[2] = &w2; waveBar[3] = &w3;
        std::vector<std::thread> th;
        for (int t = 0; t < block.x; t++)
            th.emplace_back([=]() { threadIdx = dim3(t); blockIdx = dim3(b); gridDim = grid; kernel(args...); });
        for (auto &t : th) t.join();
    }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) emu_launch(kernel, grid, block, __VA_ARGS__)
#include "kbest_frontier_sample.hip"

int main(int argc, char **argv)
{
    FILE *f = fopen(argv[1], "rb");
    int n, nSample;
    u64 seed;
    u32 base[2];
    if (fread(&n, 4, 1, f) != 1 || fread(&nSample, 4, 1, f) != 1 || fread(&seed, 8, 1, f) != 1 || fread(base, 4, 2, f) != 2) return 2;
    const long long slotDoubles = argc > 3 ? atoll(argv[3]) : (4 << 20) / 8;
    const int grid = argc > 4 ? atoi(argv[4]) : 2;
    if (n > kb::KB_FRONTIER_SAMPLE_PACK) return 2;
    kb::FrontierSamplePack pk;
    std::vector<double> sub;
    std::vector<int> keys;
    long long asgN = 0;
    int maxRows = 1;
    pk.n = n; pk.base = 0;
    for (int k = 0; k < n; k++) {
        int m, nL;
        u64 fk;
        if (fread(&m, 4, 1, f) != 1 || fread(&nL, 4, 1, f) != 1 || fread(&fk, 8, 1, f) != 1) return 2;
        const size_t sz = (size_t)(nL + m) * m;
        pk.c[k].subOff = (long long)sub.size(); pk.c[k].rowKeyOff = (long long)keys.size(); pk.c[k].asgOff = asgN;
        pk.c[k].ltOff = (long long)k * nSample; pk.c[k].frameKey = fk; pk.c[k].m = m; pk.c[k].nL = nL;
        sub.resize(sub.size() + sz);
        if (fread(sub.data() + pk.c[k].subOff, 8, sz, f) != sz) return 2;
        keys.resize(keys.size() + nL + m);
        if (fread(keys.data() + pk.c[k].rowKeyOff, 4, nL + m, f) != (size_t)(nL + m)) return 2;
        asgN += (long long)nSample * m;
        if (nL + m > maxRows) maxRows = nL + m;
    }
    fclose(f);
    // exact-size heap buffers: AddressSanitizer sees any access beyond a slot, a plan, the keys or a cluster's draws
    std::vector<double> logZ(n, -5.0), lt((size_t)n * nSample, -5.0);
    std::vector<int> info(n, -77), width(n, -77), asg((size_t)asgN, -5);
    kb::FrontierWork w;
    w.slotDoubles = slotDoubles; w.planDoubles = (long long)maxRows * kb::KB_FRONTIER_STEP_DOUBLES;
    double *layers = new double[(size_t)w.slotDoubles * grid], *plan = new double[(size_t)w.planDoubles * grid];
    w.layers = layers; w.plan = plan;
    kb::launch_frontier_sample_pack(pk, sub.data(), keys.data(), nSample, seed, base[0], asg.data(), lt.data(), logZ.data(), info.data(),
                                    width.data(), w, grid, nullptr);
    f = fopen(argv[2], "wb");
    for (int k = 0; k < n; k++) {
        fwrite(&info[k], 4, 1, f); fwrite(&width[k], 4, 1, f); fwrite(&logZ[k], 8, 1, f);
        fwrite(asg.data() + pk.c[k].asgOff, 4, (size_t)nSample * pk.c[k].m, f);
        fwrite(lt.data() + pk.c[k].ltOff, 8, nSample, f);
    }
    fclose(f);
    delete[] layers; delete[] plan;
    return 0;
}
