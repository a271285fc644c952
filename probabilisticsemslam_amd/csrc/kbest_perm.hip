// kbest_perm.hip -- permanentProb (assignment.h:13, assignment.cpp:145-290): the EXACT association probabilities of a frame, as
// ratios of matrix permanents, for frames of up to KBEST_PERM_MAX_COLS measurements.  gfx950, fp64, plain HIP C++.
//
// The reference evaluates one permanent per (landmark, measurement) pair with Nijenhuis-Wilf on the minor padded to a square
// (nwPerm.cpp): 2^(n-1) n operations per minor and a signed sum.  Here the permanent of the R x C matrix a = toProbs(cost) >= 0 is
// a sum over COLUMN SUBSETS, row by row:
//     F[0][{}] = 1,  F[i+1][S] = F[i][S] + sum_{c in S} a[i][c] F[i][S \ {c}]        (rows 0 .. i-1 fill exactly the columns S)
//     G[R][{}] = 1,  G[i][S]   = G[i+1][S] + sum_{c in S} a[i][c] G[i+1][S \ {c}]    (rows i .. R-1 fill exactly the columns S)
//     Z = F[R][all] = perm(a)
//     w[r][c] = a[r][c] sum_{S in all \ {c}} F[r][S] G[r+1][all \ {c} \ S]           (= a[r][c] perm(a without row r, column c))
//     probs[c][min(r, nL)] += w[r][c] / Z
// R 2^C C multiply-adds for ALL R C minors, every term non-negative: nothing cancels.
//
// Rows r >= nL are folded into slot nL, as every weights entry of this project does.  With the block-diagonal miss rows that
// computeQuadricCostMatrix and conditionCosts produce only row nL + c has a non-zero entry in column c, so slot nL of column c holds
// a[nL+c][c] perm(minor): the one minor the reference evaluates for the non-assignment (assignment.cpp:237-245).
//
// One workgroup per frame at a time (the grid strides over the batch; a workgroup never waits for another one).
//   * load: conditionCosts while loading when asked for (the keep rule and the column-minimum shift of assignment.cpp:439-525),
//     then toProbs (:527-542: a = exp(min - c) where min + 42 > c, else 0; min over the whole block handed to permanentProb) with
//     the exp and the expression of to_probs_kernel (kbest_costs.hip): bit for bit kbest_to_probs_f64 on the same block;
//   * rows that are zero after the gate change nothing (F[i+1] = F[i]) and are left out; zero entries skip their term (a bit mask
//     of the non-zero columns per row);
//   * forward sweep: every layer F[i] is kept -- in LDS when all of them fit beside the two G layers, else in the workgroup's slice
//     of a work space in HBM; from 13 columns on (a layer no longer fits LDS) the G layers and a live there too;
//   * backward sweep: at row r thread t adds F[r][S] G[r+1][all \ {c} \ S] over its subsets S = t, t + T, t + 2T, ... in that order
//     into one accumulator per column c; the accumulators are added over the wave (DPP, one fixed butterfly) and then over the
//     waves in ascending order by one thread per column.  T depends on the frame's OWN number of columns only (perm_threads) and
//     there are no floating-point atomics: a frame's result does not depend on the batch it travels in, bit for bit.
//   * Z == 0 (a column without a finite entry, fewer usable rows than columns): all probabilities 0 and perm = 0, not NaN.
#include <hip/hip_runtime.h>

#include <atomic>

#include "kbest_engine.h"
#include "kbest_perm_plan.h"
#include "kbest_wave.h"
#include "kbest_wave_sum.h"

namespace kb {

namespace {

// MODE 0: a, the F layers and the two G layers in LDS; 1: the F layers in the HBM work space; 2: everything there.
template <int MODE>
__global__ void __launch_bounds__(1024) kbest_perm_kernel(PermParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NWV = NT >> 6;
    const PermLds L = perm_lds(MODE, p.maxRawRow, p.maxCol);
    double *red = reinterpret_cast<double *>(smem + L.red);
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

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M;
        double *probOut = p.probs + p.probOff[b];
        const double *Cg = p.cost + p.costOff[b];
        // (uniform over the workgroup) a frame beyond what the launch was sized for is answered with perm = 0 and untouched probs
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

        for (int i = tid; i < M * (nLo + 1); i += NT) probOut[i] = 0.0;  // (rows conditionCosts drops, zero rows: exactly 0.0)

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
        // ---- toProbs (:527-542) on the block handed to permanentProb: its minimum first ----------------------------------------
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
        // (MODE 1: the sweep itself runs on the two G layers' LDS, which are idle until the backward sweep, and every layer is
        //  written to the work space on the way: nothing of the sweep waits for HBM)
        for (int S = tid; S < nsub; S += NT) {
            hist[S] = (S == 0) ? 1.0 : 0.0;
            g[S] = (S == 0) ? 1.0 : 0.0;  // G[Ra] (MODE 1: F[0] first)
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
        if (MODE == 1) {  // the LDS layers go back to the backward sweep: G[Ra]
            __syncthreads();
            for (int S = tid; S < nsub; S += NT) g[S] = (S == 0) ? 1.0 : 0.0;
            __syncthreads();
        }
        if (tid == 0 && p.perm) p.perm[b] = (Z > 0.0) ? Z : 0.0;
        if (!(Z > 0.0)) {  // (uniform) nothing to divide by: the zeros stay
            __syncthreads();
            continue;
        }

        // ---- backward sweep with the marginals ------------------------------------------------------------------------------------
        const int nt = perm_threads(M) < NT ? perm_threads(M) : NT;  // (NT >= perm_threads(M): the launch is sized by maxCol >= M)
        double missAcc = 0.0;  // thread c: slot nL of column c, rows added in descending order
        int pg = 0;
        for (int r = Ra - 1; r >= 0; r--) {
            const int kr = act[r];
            const double *ar = a + kr * M;
            const unsigned mk = maskA[kr];
            const double *Fr = hist + (long long)r * nsub;
            const double *Gc = g + (long long)pg * nsub;  // G[r+1]
            double *Gn = g + (long long)(pg ^ 1) * nsub;  // G[r]
            double *redP = red + (r & 1) * 256;
            if (tid < nt) {
                double acc[16];
#pragma unroll
                for (int c = 0; c < 16; c++) acc[c] = 0.0;
                for (int S0 = tid; S0 < nsub; S0 += PM_SPT * nt) {  // (the loads of a batch first: F[r] may live in HBM)
                    double fv[PM_SPT];
#pragma unroll
                    for (int j = 0; j < PM_SPT; j++) fv[j] = (S0 + j * nt < nsub) ? Fr[S0 + j * nt] : 0.0;
#pragma unroll
                    for (int j = 0; j < PM_SPT; j++) {
                        const double f = fv[j];
                        if (f == 0.0) continue;
                        const unsigned S = (unsigned)(S0 + j * nt);
                        const unsigned cols = mk & ~S;
                        const unsigned comp = full ^ S;
#pragma unroll
                        for (int c = 0; c < 16; c++)
                            if ((cols >> c) & 1u) acc[c] = acc[c] + f * Gc[comp ^ (1u << c)];
                    }
                }
#pragma unroll
                for (int c = 0; c < 16; c++)
                    if ((mk >> c) & 1u) {  // (uniform)
                        const double s = wave_sum63_f64(acc[c]);
                        if (lane == 63) redP[wave * 16 + c] = s;
                    }
            }
            if (r > 0) {
                const int left = Ra - r;  // rows r .. Ra-1
                for (int S = tid; S < nsub; S += NT) {
                    double v = 0.0;
                    if (__popc(S) <= left) {
                        v = Gc[S];
                        unsigned cols = (unsigned)S & mk;
                        while (cols) {
                            const int c = __ffs(cols) - 1;
                            cols &= cols - 1u;
                            v = v + ar[c] * Gc[S ^ (1 << c)];
                        }
                    }
                    Gn[S] = v;
                }
            }
            __syncthreads();
            if (tid < M && ((mk >> tid) & 1u)) {
                double s = redP[tid];
                for (int w = 1; w < (nt >> 6); w++) s = s + redP[w * 16 + tid];
                const double wv = ar[tid] * s;
                const int raw = rawRow[kr];
                if (raw < nLo) probOut[tid * (nLo + 1) + raw] = wv / Z;  // scatter back to the caller's landmark numbering (:68-74)
                else missAcc = missAcc + wv;
            }
            pg ^= 1;
        }
        if (tid < M) probOut[tid * (nLo + 1) + nLo] = missAcc / Z;
        __syncthreads();
    }
}

template <int MODE>
hipError_t launch_mode(const PermParams &p, int grid, int threads, int lds, hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_perm_kernel<MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((kbest_perm_kernel<MODE>), dim3(grid), dim3(threads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

PermPlan perm_plan(int maxRawRow, int maxCol, int ldsLimit, int ldsPerCU)
{
    PermPlan pl;
    pl.threads = perm_threads(maxCol);
    // all layers in LDS where four frames still share a CU; else the two G layers and a; else (a layer of 13 columns is 64 KiB) HBM
    const int lds0 = maxCol <= 12 ? perm_lds(0, maxRawRow, maxCol).total : 1 << 30;
    const int lds1 = maxCol <= 12 ? perm_lds(1, maxRawRow, maxCol).total : 1 << 30;
    if (lds0 <= ldsLimit && lds0 <= ldsPerCU / 4) { pl.mode = 0; pl.lds = lds0; }
    else if (lds1 <= ldsLimit) { pl.mode = 1; pl.lds = lds1; }
    else { pl.mode = 2; pl.lds = perm_lds(2, maxRawRow, maxCol).total; }
    pl.slotDoubles = pl.mode == 0 ? 0 : (long long)maxRawRow * maxCol + ((long long)(maxRawRow + 2) << maxCol);
    return pl;
}

hipError_t launch_kbest_perm(const PermParams &p, const PermPlan &pl, int grid, hipStream_t stream)
{
    return pl.mode == 0 ? launch_mode<0>(p, grid, pl.threads, pl.lds, stream)
         : pl.mode == 1 ? launch_mode<1>(p, grid, pl.threads, pl.lds, stream)
                        : launch_mode<2>(p, grid, pl.threads, pl.lds, stream);
}

}  // namespace kb
