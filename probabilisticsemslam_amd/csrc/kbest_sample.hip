// kbest_sample.hip -- joint associations DRAWN from the exact posterior of a frame of up to KBEST_PERM_MAX_COLS measurements (not in
// the reference, whose permOpt 0 only estimates the permanent by sampling).  gfx950, fp64, plain HIP C++.  DESIGN.md section 16.
//
// The forward layers of kbest_perm.hip, F[i+1][S] = F[i][S] + sum_{c in S} a[i][c] F[i][S \ {c}], list the weights of the choices of
// row i given that rows 0 .. i fill exactly the columns S: row i stays unassigned (F[i][S]) or takes column c (a[i][c] F[i][S \ c]).
// Walking the layers backwards from (Ra, all) and choosing one term per row in proportion gives a joint association with
// probability (product of the chosen a) / Z exactly: independent draws, no rejection, no burn-in.
//
// One workgroup per frame at a time (the grid strides over the batch; a workgroup never waits for another one).
//   * load and forward sweep: kbest_perm_kernel's, restated expression for expression (that kernel keeps its own lines and with them
//     its code, bit for bit): conditionCosts while loading when asked for, toProbs, the active rows and their column masks, every
//     layer F[0] .. F[Ra-1] kept by the same three modes of the same perm_plan, Z = F[Ra][all] by the same expression.  perm[b]
//     carries the bits of kbest_permanent_probs_batch_f64's perm[b].
//   * walk: thread t draws samples s = t, t + NT, ...  State S = all; for i = Ra-1 .. 0 while S is not empty: tot = F[i+1][S]
//     (Z at i = Ra-1), T = u(s, i) tot, acc = F[i][S]; T < acc: row i stays unassigned; else for c ascending in S & mask_i:
//     acc = acc + a[i][c] F[i][S \ c], the first c with T < acc is taken (rounding lets the walk fall through: the last c whose
//     term was > 0).  acc runs through the additions that made F[i+1][S], in their order: its last value IS tot.  A state (i, S)
//     is only ever entered through a term > 0, so F[i+1][S] > 0 there, and since F[i][S] = 0 whenever S has more columns than rows
//     remain, forced assignments need no special case and S is empty when the walk ends: every column is written.
//   * u(s, i): Philox4x32-10, no state, no buffer: key (seed low, seed high), counter (sampleBase + s, i >> 1, frameKey[b] low,
//     frameKey[b] high) with i the index among the ACTIVE rows; output words 0, 1 serve even i, words 2, 3 odd i;
//     u = (((hi << 32) | lo) >> 11) 2^-53 with lo the first and hi the second word of the pair.  A frame's draws depend on its
//     key, not on the batch it travels in, and not on whether the caller or the kernel conditioned the block.
//   * out: assign[s][c] = the RAW row of the caller's block that column c takes (a miss is the column's own row >= nL, not folded),
//     logProb[s] = log(prod a) - log Z.  Z == 0: every assign -1, logProb NaN, perm 0.
// No floating-point atomics, no grid barrier, no flag.
#include <hip/hip_runtime.h>

#include <atomic>

#include "kbest_engine.h"
#include "kbest_perm_plan.h"
#include "kbest_wave.h"

#ifndef KB_DYNAMIC_LDS  // (tests/cpp/sample_host.cpp runs these lines on the host, on a heap block of exactly the planned size)
#define KB_DYNAMIC_LDS(name) extern __shared__ __align__(16) unsigned char name[]
#endif

namespace kb {

namespace {

struct Philox4 { u32 w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1)
{
    for (int round = 0; round < 10; round++) {
        const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
        const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
        c1 = (u32)p1;
        c3 = (u32)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// MODE 0: a and the F layers in LDS; 1: the F layers in the HBM work space (the sweep on two LDS layers); 2: everything there.
template <int MODE>
__global__ void __launch_bounds__(1024) kbest_sample_kernel(SampleParams p)
{
    KB_DYNAMIC_LDS(smem);
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NWV = NT >> 6;
    const PermLds L = perm_lds(MODE, p.maxRawRow, p.maxCol);
    double *colMin = reinterpret_cast<double *>(smem + L.colMin);
    double *waveMin = reinterpret_cast<double *>(smem + L.waveMin);
    double *blockMin = reinterpret_cast<double *>(smem + L.ctl);
    int *nKeptW = reinterpret_cast<int *>(smem + L.ctl + 8);
    int *nActW = nKeptW + 1;
    unsigned short *rawRow = reinterpret_cast<unsigned short *>(smem + L.rawRow);
    unsigned short *maskA = reinterpret_cast<unsigned short *>(smem + L.mask);
    unsigned short *act = reinterpret_cast<unsigned short *>(smem + L.act);
    double *slice = p.work + (long long)blockIdx.x * p.slotStride;  // this workgroup's part of the work space (MODE > 0)
    const double INF = d_inf();
    const u32 k0 = (u32)p.seed, k1 = (u32)(p.seed >> 32);

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M;
        const double *Cg = p.cost + p.costOff[b];
        // (uniform over the workgroup) a frame beyond what the launch was sized for is answered with perm = 0, nothing else written
        if (M < 1 || M > p.maxCol || M > 16 || nLo < 0 || NR > p.maxRawRow) {
            if (tid == 0 && p.perm) p.perm[b] = 0.0;
            continue;
        }
        const int nsub = 1 << M;
        const unsigned full = (unsigned)nsub - 1u;
        double *a, *g, *hist;
        if constexpr (MODE < 2) {
            a = reinterpret_cast<double *>(smem + L.a);
            g = reinterpret_cast<double *>(smem + L.g);
        } else {
            a = slice;
            g = slice + (long long)p.maxRawRow * p.maxCol;
        }
        if constexpr (MODE < 1) hist = reinterpret_cast<double *>(smem + L.hist);
        else hist = slice + (long long)p.maxRawRow * p.maxCol + (2ll << p.maxCol);

        // ---- conditionCosts (assignment.cpp:439-525) while loading ------------------------------------------------------------
        int N;
        if (p.condition) {
            for (int c = wave; c < M; c += NWV) {  // column minima (:450-458)
                double m = INF;
                for (int r = lane; r < NR; r += 64) m = min_keep(m, Cg[(long long)c * NR + r]);
                m = wave_min_f64(m);
                if (lane == 0) colMin[c] = m;
            }
            __syncthreads();
            for (int r = tid; r < NR; r += NT) {  // a row is kept iff some entry is within 42 of its column's minimum (:462-474)
                bool good = false;
                for (int c = 0; c < M; c++) good = good | (Cg[(long long)c * NR + r] <= colMin[c] + PM_GATE);
                maskA[r] = good ? 1 : 0;
            }
            __syncthreads();
            if (wave == 0) {  // kept rows compacted in order (:481-486)
                int n = 0;
                for (int base = 0; base < NR; base += 64) {
                    const int r = base + lane;
                    const bool good = r < NR && maskA[r] != 0;
                    const u64 m = __ballot(good);
                    if (good) rawRow[n + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)r;
                    n += __popcll(m);
                }
                if (lane == 0) *nKeptW = n;
            }
            __syncthreads();
            N = *nKeptW;
        } else {
            for (int r = tid; r < NR; r += NT) rawRow[r] = (unsigned short)r;
            N = NR;
            __syncthreads();
        }
        // ---- toProbs (:527-542) on the conditioned block: its minimum first ------------------------------------------------------
        {
            double m = INF;
            for (int i = tid; i < N * M; i += NT) {
                const int r = i / M, c = i - r * M;
                double x = Cg[(long long)c * NR + rawRow[r]];
                if (p.condition) x = (x <= colMin[c] + PM_GATE) ? (x - colMin[c]) : INF;  // (:490-494)
                a[i] = x;
                m = min_keep(m, x);
            }
            m = wave_min_f64(m);
            if (lane == 0) waveMin[wave] = m;
            __syncthreads();
            if (tid == 0) {
                double mm = waveMin[0];
                for (int w = 1; w < NWV; w++) mm = min_keep(mm, waveMin[w]);
                *blockMin = mm;
            }
            __syncthreads();
            const double mn = *blockMin;
            for (int i = tid; i < N * M; i += NT) {
                const double c = a[i];
                a[i] = (mn + PM_GATE > c) ? exp(mn - c) : 0.0;  // :536-540, as to_probs_kernel has it
            }
            __syncthreads();
            for (int r = tid; r < N; r += NT) {  // the non-zero columns of every row
                unsigned mk = 0;
                for (int c = 0; c < M; c++) mk |= (a[r * M + c] > 0.0) ? (1u << c) : 0u;
                maskA[r] = (unsigned short)mk;
            }
            __syncthreads();
            if (wave == 0) {  // rows that are zero after the gate are left out
                int n = 0;
                for (int base = 0; base < N; base += 64) {
                    const int r = base + lane;
                    const bool on = r < N && maskA[r] != 0;
                    const u64 m2 = __ballot(on);
                    if (on) act[n + __popcll(m2 & ((1ull << lane) - 1ull))] = (unsigned short)r;
                    n += __popcll(m2);
                }
                if (lane == 0) *nActW = n;
            }
            __syncthreads();
        }
        const int Ra = *nActW;

        // ---- forward sweep: hist[i] = F[i] over the active rows, i = 0 .. Ra - 1 -------------------------------------------------
        // (MODE 1: the sweep itself runs on two layers in LDS and every layer is written to the work space on the way: nothing of
        //  the sweep waits for HBM)
        for (int S = tid; S < nsub; S += NT) {
            hist[S] = (S == 0) ? 1.0 : 0.0;
            if (MODE == 1) g[S] = (S == 0) ? 1.0 : 0.0;
        }
        __syncthreads();
        int pf = 0;
        for (int i = 0; i + 1 < Ra; i++) {
            const int kr = act[i];
            const double *ar = a + kr * M;
            const unsigned mk = maskA[kr];
            const double *Fi = (MODE == 1) ? g + (long long)pf * nsub : hist + (long long)i * nsub;
            double *Fo = hist + (long long)(i + 1) * nsub;
            double *Fl = g + (long long)(pf ^ 1) * nsub;
            for (int S = tid; S < nsub; S += NT) {
                double v = 0.0;
                if (__popc(S) <= i + 1) {  // (more columns than rows so far: 0)
                    v = Fi[S];
                    unsigned cols = (unsigned)S & mk;
                    while (cols) {
                        const int c = __ffs(cols) - 1;
                        cols &= cols - 1u;
                        v = v + ar[c] * Fi[S ^ (1 << c)];
                    }
                }
                Fo[S] = v;
                if (MODE == 1) Fl[S] = v;
            }
            pf ^= 1;
            __syncthreads();
        }
        double Z = 0.0;
        if (Ra >= M) {  // Z = F[Ra][all], by the same expression
            const int kr = act[Ra - 1];
            const double *ar = a + kr * M;
            const double *Fi = (MODE == 1) ? g + (long long)pf * nsub : hist + (long long)(Ra - 1) * nsub;
            Z = Fi[full];
            unsigned cols = full & maskA[kr];
            while (cols) {
                const int c = __ffs(cols) - 1;
                cols &= cols - 1u;
                Z = Z + ar[c] * Fi[full ^ (1u << c)];
            }
        }
        if (tid == 0 && p.perm) p.perm[b] = (Z > 0.0) ? Z : 0.0;
        int *asg = p.assign + p.asgOff[b];
        double *lp = p.logProb + p.lpOff[b];
        if (!(Z > 0.0)) {  // (uniform) no joint association has a weight
            for (long long i = tid; i < (long long)p.nSample * M; i += NT) asg[i] = -1;
            for (int s = tid; s < p.nSample; s += NT) lp[s] = __longlong_as_double(0x7ff8000000000000LL);
            __syncthreads();
            continue;
        }
        __syncthreads();

        // ---- the walk: one sample per thread at a time --------------------------------------------------------------------------
        const u64 fk = p.frameKey ? p.frameKey[b] : (u64)b;
        const u32 f0 = (u32)fk, f1 = (u32)(fk >> 32);
        const double logZ = log(Z);
        for (int s = tid; s < p.nSample; s += NT) {
            int *row = asg + (long long)s * M;
            unsigned S = full;
            double prod = 1.0;
            Philox4 rnd = {};
            for (int i = Ra - 1; i >= 0 && S != 0u; i--) {
                if ((i & 1) || i == Ra - 1) rnd = philox4x32_10(p.sampleBase + (u32)s, (u32)(i >> 1), f0, f1, k0, k1);
                const u32 lo = (i & 1) ? rnd.w[2] : rnd.w[0], hi = (i & 1) ? rnd.w[3] : rnd.w[1];
                const double u = (double)((((u64)hi << 32) | lo) >> 11) * 0x1.0p-53;
                const double *Fi = hist + (long long)i * nsub;
                const double tot = (i == Ra - 1) ? Z : Fi[nsub + S];  // F[i+1][S]
                const double T = u * tot;
                double acc = Fi[S];
                if (T < acc) continue;  // row i stays unassigned
                const int kr = act[i];
                const double *ar = a + kr * M;
                unsigned cols = S & maskA[kr];
                int take = -1;
                double at = 1.0;
                while (cols) {
                    const int c = __ffs(cols) - 1;
                    cols &= cols - 1u;
                    const double term = ar[c] * Fi[S ^ (1u << c)];
                    acc = acc + term;
                    if (term > 0.0) { take = c; at = ar[c]; }
                    if (T < acc) break;
                }
                if (take >= 0) {
                    row[take] = rawRow[kr];
                    S ^= 1u << take;
                    prod = prod * at;
                }
            }
            lp[s] = log(prod) - logZ;
        }
        __syncthreads();
    }
}

template <int MODE>
hipError_t launch_mode(const SampleParams &p, int grid, int threads, int lds, hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_sample_kernel<MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((kbest_sample_kernel<MODE>), dim3(grid), dim3(threads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_kbest_sample(const SampleParams &p, const PermPlan &pl, int grid, hipStream_t stream)
{
    return pl.mode == 0 ? launch_mode<0>(p, grid, pl.threads, pl.lds, stream)
         : pl.mode == 1 ? launch_mode<1>(p, grid, pl.threads, pl.lds, stream)
                        : launch_mode<2>(p, grid, pl.threads, pl.lds, stream);
}

}  // namespace kb
