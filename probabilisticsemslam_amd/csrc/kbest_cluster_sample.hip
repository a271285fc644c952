// kbest_cluster_sample.hip -- joint associations DRAWN from the exact posterior of a gated frame of up to KBEST_CLUSTER_MAX_COLS
// measurements whose clusters have at most KBEST_CLUSTER_MAX_SIZE: one backward walk per cluster, the joints concatenated.
// gfx950, fp64, plain HIP C++.  DESIGN.md section 17.
//
// The posterior of a gated frame is the product of its clusters' posteriors (kbest_cluster.hip), so a walk of kbest_sample.hip on
// every cluster's own forward layers F_k, with the joints concatenated, is an exact, independent draw of the frame.  The uniform of
// a decision stays u(s, i) with i the index of the row among the frame's ACTIVE rows: the whole-frame layers factorise over the
// clusters, the ratio that decides row i is the ratio inside its cluster, and on a frame kbest_sample.hip takes the decisions are
// the same function of the same uniforms.
//
// One workgroup per frame at a time (the grid strides over the batch; a workgroup never waits for another one).
//   * prologue: kbest_cluster_kernel's, restated expression for expression (that kernel keeps its own lines and with them its code,
//     bit for bit): conditionCosts while loading, the block minimum, the gate, the row masks, the active rows, labelling by integer
//     atomicMin, rows sorted by cluster -- and beside rowList the index of every sorted row among the active rows (rowAct);
//   * clusters in label order.  A run of up to NWV consecutive SMALL clusters (cs_small: cl_small) is built side by side, one wave
//     each, by the small tier's forward sweep (the layer in a register per lane, the history in the wave's 4 KiB); after one
//     barrier every thread walks those clusters in label order.  Every other cluster is swept by the whole workgroup with the
//     forward sweep of kbest_perm.hip (layers in the LDS arena where they fit, else in the workgroup's slot of the work space: the
//     same instructions on either) and then walked.  No backward sweep;
//   * the walk (kbest_cluster_sample.h): thread t owns draws s = t, t + NT, ... for EVERY cluster of the frame, so the running sum
//     logProb[s] = sum_k (log prod_k a - log Z_k), one term per cluster added left to right from 0.0, lives in the caller's buffer
//     without atomics.  No product over the whole frame is formed;
//   * out: assign[s][c] = the RAW row of the caller's block (a miss is the column's own row >= nL, not folded); logPerm, info,
//     maxCluster as kbest_cluster_kernel writes them.  A cluster of more than 16 columns: info = -2; layers beyond the slot: -3;
//     both: assign -1, logProb NaN, logPerm NaN.  Some Z_k == 0: assign -1, logProb NaN, logPerm -inf, info 0.  A frame beyond the
//     launch's bounds: info = -1 and nothing else is touched.
// No floating-point atomics, no grid barrier, no flag, no sum over threads: a frame's outputs are a function of (seed, frame key,
// draw index, frame) alone, whatever the batch, the launch's bounds, the workgroup's size or the caps.
#include <hip/hip_runtime.h>

#include <atomic>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_cluster_sample.h"

namespace kb {

namespace {

// ---- kbest_cluster.hip's constants and helpers, restated: that file stays as it is ------------------------------------------------
constexpr double CS_GATE = 42.0;  // assignment.cpp:9
constexpr int CS_MAX_COLS = 128;  // KBEST_CLUSTER_MAX_COLS: two mask words per row
constexpr int CS_MAX_SIZE = 16;   // KBEST_CLUSTER_MAX_SIZE

// the j-th set bit (ascending) of a 128-bit mask that has more than j bits
__device__ __forceinline__ int cs_nth_bit128(u64 lo, u64 hi, int j)
{
    for (int t = 0; t < j; t++) {
        if (lo) lo &= lo - 1ull;
        else hi &= hi - 1ull;
    }
    return lo ? __ffsll((unsigned long long)lo) - 1 : 64 + __ffsll((unsigned long long)hi) - 1;
}

// cl_lds of kbest_cluster.hip, field for field and byte for byte (cluster_plan sizes the launch with it).  What the sampler does
// not need it uses for its own: red (the marginal sums' scratch) holds Z of every cluster and the columns of the small clusters
// being walked; flag is free once the active rows are compacted and then holds rowAct; locMask serves the forward sweep.
struct CsLds {
    int red, colMin, waveMin, ctl, logZ, label, csize, crows, cstart, clist, ccol, rawRow, flag, act, rowRoot, rowList, locMask, maskLo,
        maskHi, arena, total;
};

__host__ __device__ inline CsLds cs_lds(int maxRawRow, int maxCol, int arenaBytes)
{
    CsLds l;
    int o = 0;
    l.red = o;     o += 2 * 16 * 16 * 8;  // double Z[128]; int wcol[16][8]
    l.colMin = o;  o += maxCol * 8;
    l.waveMin = o; o += 16 * 8;
    l.ctl = o;     o += 48;               // double blockMin; int nKept, nAct, nClus, maxC, refuse, bad
    l.logZ = o;    o += maxCol * 8;       // [cluster]
    const int cols4 = (4 * maxCol + 7) & ~7;
    l.label = o;   o += cols4;            // int: the label of every column
    l.csize = o;   o += cols4;            // int [root]: columns of the cluster
    l.crows = o;   o += cols4;            // int [root]: rows of the cluster
    l.cstart = o;  o += cols4;            // int [root]: its first entry of rowList
    l.clist = o;   o += cols4;            // int [cluster]: the roots in ascending order
    l.ccol = o;    o += 16 * 4;           // int: the columns of the cluster the workgroup works on
    const int rows2 = (2 * maxRawRow + 7) & ~7;
    l.rawRow = o;  o += rows2;            // u16: raw row of every kept row
    l.flag = o;    o += rows2;            // u16: row kept / row active; then rowAct: the active index of every entry of rowList
    l.act = o;     o += rows2;            // u16: kept index of every active (non-zero) row
    l.rowRoot = o; o += rows2;            // u16: the root of every active row
    l.rowList = o; o += rows2;            // u16: kept indices sorted by cluster
    l.locMask = o; o += rows2;            // u16: non-zero columns of the rows of the cluster the workgroup works on
    l.maskLo = o;  o += maxRawRow * 8;    // u64: non-zero columns 0..63 of every kept row
    l.maskHi = o;  o += maxRawRow * 8;    // ... and 64..127
    o = (o + 15) & ~15;
    l.arena = o;   o += arenaBytes;       // the small tier: CS_WAVE_BYTES per wave; the workgroup tier: a, F layers
    l.total = (o + 15) & ~15;
    return l;
}

// one entry of a: conditionCosts (assignment.cpp:490-494) and toProbs (:536-540) on the raw cost, as to_probs_kernel has it
__device__ __forceinline__ double cs_entry(const double *Cg, int NR, int c, int raw, bool condition, const double *colMin, double mn)
{
    double x = Cg[(long long)c * NR + raw];
    if (condition) x = (x <= colMin[c] + CS_GATE) ? (x - colMin[c]) : d_inf();
    return (mn + CS_GATE > x) ? exp(mn - x) : 0.0;
}

// ... and whether it is non-zero: the gate alone (exp of more than -42 is positive)
__device__ __forceinline__ bool cs_nonzero(const double *Cg, int NR, int c, int raw, bool condition, const double *colMin, double mn)
{
    double x = Cg[(long long)c * NR + raw];
    if (condition) x = (x <= colMin[c] + CS_GATE) ? (x - colMin[c]) : d_inf();
    return mn + CS_GATE > x;
}

// This file is compiled twice.  On its own: kbest_clustered_sample_assoc_batch_f64_dev's kernel.  Through
// kbest_cluster_sample_partial.hip, which defines KB_CLUSTER_SAMPLE_PARTIAL and includes it
// (kbest_hybrid_frontier_sample_assoc_batch_f64): a cluster of more than maxExact columns, or whose layers exceed the slot, is OPEN
// as in kbest_cluster.hip's partial mode -- it does not refuse the frame, its columns stay -1, it adds no term to logProb or
// logPerm and takes no place among the clusters; every other cluster is drawn by the same sweeps and the same walk with the same
// uniforms.  A translation unit of its own, so that the plain kernel's code stays what it is, register for register.
#ifdef KB_CLUSTER_SAMPLE_PARTIAL
constexpr bool CS_PARTIAL = true;
#define CS_KERNEL kbest_cluster_sample_partial_kernel(ClusterSampleParams p, int maxExact)
#else
constexpr bool CS_PARTIAL = false;
#define CS_KERNEL kbest_cluster_sample_kernel(ClusterSampleParams p)
#endif

__global__ void __launch_bounds__(512) CS_KERNEL
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NWV = NT >> 6;
    const CsLds L = cs_lds(p.maxRawRow, p.maxCol, p.arenaBytes);
    double *Zs = reinterpret_cast<double *>(smem + L.red);          // [cluster]
    int *wcol = reinterpret_cast<int *>(smem + L.red + 128 * 8);    // [wave][8]: the columns of the small clusters being walked
    double *colMin = reinterpret_cast<double *>(smem + L.colMin);
    double *waveMin = reinterpret_cast<double *>(smem + L.waveMin);
    double *blockMin = reinterpret_cast<double *>(smem + L.ctl);
    int *ctl = reinterpret_cast<int *>(smem + L.ctl + 8);  // nKept, nAct, nClus, maxC, refuse, bad
    double *logZ = reinterpret_cast<double *>(smem + L.logZ);
    int *label = reinterpret_cast<int *>(smem + L.label);
    int *csize = reinterpret_cast<int *>(smem + L.csize);
    int *crows = reinterpret_cast<int *>(smem + L.crows);
    int *cstart = reinterpret_cast<int *>(smem + L.cstart);
    int *clist = reinterpret_cast<int *>(smem + L.clist);
    int *ccol = reinterpret_cast<int *>(smem + L.ccol);
    unsigned short *rawRow = reinterpret_cast<unsigned short *>(smem + L.rawRow);
    unsigned short *flag = reinterpret_cast<unsigned short *>(smem + L.flag);
    unsigned short *rowAct = flag;  // (free once act is compacted)
    unsigned short *act = reinterpret_cast<unsigned short *>(smem + L.act);
    unsigned short *rowRoot = reinterpret_cast<unsigned short *>(smem + L.rowRoot);
    unsigned short *rowList = reinterpret_cast<unsigned short *>(smem + L.rowList);
    unsigned short *locMask = reinterpret_cast<unsigned short *>(smem + L.locMask);
    u64 *maskLo = reinterpret_cast<u64 *>(smem + L.maskLo);
    u64 *maskHi = reinterpret_cast<u64 *>(smem + L.maskHi);
    double *arena = reinterpret_cast<double *>(smem + L.arena);
    double *slice = p.work + (long long)blockIdx.x * p.slotStride;  // this workgroup's part of the work space
    const long long aPart = (long long)p.maxRawRow * CS_MAX_SIZE;   // ... its first doubles: a of a cluster; then the layers
    const double INF = d_inf();
    const double QNAN = __longlong_as_double(0x7ff8000000000000LL);
    const bool cond = p.condition != 0;
    const u32 k0 = (u32)p.seed, k1 = (u32)(p.seed >> 32);

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M;
        const double *Cg = p.cost + p.costOff[b];
        // (uniform over the workgroup) a frame beyond what the launch was sized for: info = -1 and nothing else is touched
        if (M < 1 || M > p.maxCol || M > CS_MAX_COLS || nLo < 0 || NR > p.maxRawRow) {
            if (tid == 0 && p.info) p.info[b] = -1;
            continue;
        }
        int *asg = p.assign + p.asgOff[b];
        double *lp = p.logProb + p.lpOff[b];

        // ---- conditionCosts (assignment.cpp:439-525) while loading: as kbest_perm.hip has it --------------------------------------
        int N;
        if (cond) {
            for (int c = wave; c < M; c += NWV) {  // column minima (:450-458)
                double m = INF;
                for (int r = lane; r < NR; r += 64) m = min_keep(m, Cg[(long long)c * NR + r]);
                m = wave_min_f64(m);
                if (lane == 0) colMin[c] = m;
            }
            __syncthreads();
            for (int r = tid; r < NR; r += NT) {  // a row is kept iff some entry is within 42 of its column's minimum (:462-474)
                bool good = false;
                for (int c = 0; c < M; c++) good = good | (Cg[(long long)c * NR + r] <= colMin[c] + CS_GATE);
                flag[r] = good ? 1 : 0;
            }
            __syncthreads();
            if (wave == 0) {  // kept rows compacted in order (:481-486)
                int n = 0;
                for (int base = 0; base < NR; base += 64) {
                    const int r = base + lane;
                    const bool good = r < NR && flag[r] != 0;
                    const u64 m = __ballot(good);
                    if (good) rawRow[n + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)r;
                    n += __popcll(m);
                }
                if (lane == 0) ctl[0] = n;
            }
            __syncthreads();
            N = ctl[0];
        } else {
            for (int r = tid; r < NR; r += NT) rawRow[r] = (unsigned short)r;
            N = NR;
            __syncthreads();
        }
        // ---- toProbs (:527-542) on the block handed over: its minimum first, then the non-zero columns of every row -------------
        {
            double m = INF;
            for (int i = tid; i < N * M; i += NT) {
                const int c = i / N, r = i - c * N;
                double x = Cg[(long long)c * NR + rawRow[r]];
                if (cond) x = (x <= colMin[c] + CS_GATE) ? (x - colMin[c]) : INF;  // (:490-494)
                m = min_keep(m, x);
            }
            m = wave_min_f64(m);
            if (lane == 0) waveMin[wave] = m;
            __syncthreads();
            if (tid == 0) {
                double mm = waveMin[0];
                for (int w = 1; w < NWV; w++) mm = min_keep(mm, waveMin[w]);
                *blockMin = mm;
                ctl[5] = 0;  // bad
            }
            __syncthreads();
        }
        const double mn = *blockMin;
        for (int r = tid; r < N; r += NT) {
            const int raw = rawRow[r];
            u64 lo = 0, hi = 0;
            for (int c = 0; c < M; c++) {
                const bool nz = cs_nonzero(Cg, NR, c, raw, cond, colMin, mn);
                if (c < 64) lo |= nz ? bit64(c) : 0ull;
                else hi |= nz ? bit64(c) : 0ull;
            }
            maskLo[r] = lo;
            maskHi[r] = hi;
            flag[r] = (lo | hi) ? 1 : 0;
        }
        for (int c = tid; c < M; c += NT) {
            label[c] = c;
            csize[c] = 0;
            crows[c] = 0;
        }
        __syncthreads();
        if (wave == 0) {  // rows that are zero after the gate are left out
            int n = 0;
            for (int base = 0; base < N; base += 64) {
                const int r = base + lane;
                const bool on = r < N && flag[r] != 0;
                const u64 m2 = __ballot(on);
                if (on) act[n + __popcll(m2 & ((1ull << lane) - 1ull))] = (unsigned short)r;
                n += __popcll(m2);
            }
            if (lane == 0) ctl[1] = n;
        }
        __syncthreads();
        const int Ra = ctl[1];

        // ---- labelling: the lowest column of every connected component ---------------------------------------------------------
        for (int sweep = 0; sweep <= M; sweep++) {  // (a label travels at least one column further per sweep)
            int changed = 0;
            for (int i = tid; i < Ra; i += NT) {
                const int kr = act[i];
                const u64 lo = maskLo[kr], hi = maskHi[kr];
                int m = CS_MAX_COLS;
                for (u64 w = lo; w; w &= w - 1ull) m = min(m, label[__ffsll((unsigned long long)w) - 1]);
                for (u64 w = hi; w; w &= w - 1ull) m = min(m, label[64 + __ffsll((unsigned long long)w) - 1]);
                for (u64 w = lo; w; w &= w - 1ull) changed |= atomicMin(&label[__ffsll((unsigned long long)w) - 1], m) > m;
                for (u64 w = hi; w; w &= w - 1ull) changed |= atomicMin(&label[64 + __ffsll((unsigned long long)w) - 1], m) > m;
            }
            if (!__syncthreads_or(changed)) break;
        }
        // ---- the clusters: their columns, their rows (sorted by cluster, in row order inside one) ----------------------------------
        for (int c = tid; c < M; c += NT) atomicAdd(&csize[label[c]], 1);
        for (int i = tid; i < Ra; i += NT) {
            const int kr = act[i];
            const u64 lo = maskLo[kr], hi = maskHi[kr];
            const int fc = lo ? __ffsll((unsigned long long)lo) - 1 : 64 + __ffsll((unsigned long long)hi) - 1;
            const int root = label[fc];
            rowRoot[i] = (unsigned short)root;
            atomicAdd(&crows[root], 1);
        }
        __syncthreads();
        if (tid == 0) {  // (at most 128 columns: one thread)
            int n = 0, at = 0, maxC = 0, refuse = 0;
            for (int c = 0; c < M; c++)
                if (label[c] == c) {
                    const int m = csize[c], R = crows[c];
                    clist[n++] = c;
                    cstart[c] = at;
                    at += R;
                    if (m > maxC) maxC = m;
#ifdef KB_CLUSTER_SAMPLE_PARTIAL
                    if (m > maxExact || ((long long)(R + 2) << m) * 8 > p.slotBytes) n--;  // open: no place in clist
#else
                    if (m > CS_MAX_SIZE) refuse = -2;
                    else if (refuse == 0 && ((long long)(R + 2) << m) * 8 > p.slotBytes) refuse = -3;
#endif
                }
            ctl[2] = n;
            ctl[3] = maxC;
            ctl[4] = refuse;
        }
        __syncthreads();
        const int nClus = ctl[2], refuse = ctl[4];
        if (tid == 0 && p.maxCluster) p.maxCluster[b] = ctl[3];
        if (refuse != 0) {  // (uniform) no draw: every thread answers the draws it owns
            for (int s = tid; s < p.nSample; s += NT) {
                for (int c = 0; c < M; c++) asg[(long long)s * M + c] = -1;
                lp[s] = QNAN;
            }
            if (tid == 0) {
                if (p.info) p.info[b] = refuse;
                if (p.logPerm) p.logPerm[b] = QNAN;
            }
            __syncthreads();
            continue;
        }
        for (int i = tid; i < Ra; i += NT) {
            const int root = rowRoot[i];
            int rank = 0;
            for (int j = 0; j < i; j++) rank += (rowRoot[j] == root) ? 1 : 0;
            rowList[cstart[root] + rank] = act[i];
            rowAct[cstart[root] + rank] = (unsigned short)i;  // the i of u(s, i): the row's index among the frame's active rows
        }
        for (int s = tid; s < p.nSample; s += NT) lp[s] = 0.0;  // (its owner's running sum)
        if constexpr (CS_PARTIAL)
            for (int s = tid; s < p.nSample; s += NT)  // (its owner: the columns of the open clusters stay so)
                for (int c = 0; c < M; c++) asg[(long long)s * M + c] = -1;
        __syncthreads();

        const u64 fk = p.frameKey ? p.frameKey[b] : (u64)b;
        const u32 f0 = (u32)fk, f1 = (u32)(fk >> 32);

        // ---- the clusters in label order ------------------------------------------------------------------------------------------
        int k = 0;
        while (k < nClus) {  // (uniform)
            const int root = clist[k], m = csize[root], R = crows[root], st = cstart[root];
            if (cs_small(m, R)) {
                // ---- a run of small clusters: one wave each, side by side; then every thread walks them in label order -----------
                int n = 1;
                while (n < NWV && k + n < nClus && cs_small(csize[clist[k + n]], crows[clist[k + n]])) n++;
                if (wave < n) {
                    const int kk = k + wave, rootW = clist[kk], mW = csize[rootW], RW = crows[rootW], stW = cstart[rootW];
                    const int nsub = 1 << mW, full = nsub - 1;
                    const u64 b0 = __ballot(lane < M && label[lane < M ? lane : 0] == rootW);
                    const u64 b1 = __ballot(64 + lane < M && label[64 + lane < M ? 64 + lane : 0] == rootW);
                    const int colj = lane < mW ? cs_nth_bit128(b0, b1, lane) : 0;
                    const bool inS = lane < nsub;
                    double *hist = arena + wave * (CS_WAVE_BYTES / 8);  // [R][nsub]: lane S writes its own entries only
                    double *aSt = hist + RW * nsub;                     // [R][m]: lane j likewise
                    double f = lane == 0 ? 1.0 : 0.0;                   // F[i][S] in lane S
                    if (lane < mW) wcol[wave * 8 + lane] = colj;
                    for (int i = 0; i < RW; i++) {
                        const int raw = rawRow[rowList[stW + i]];
                        double av = 0.0;
                        if (lane < mW) {
                            av = cs_entry(Cg, NR, colj, raw, cond, colMin, mn);
                            aSt[i * mW + lane] = av;
                        }
                        if (inS) hist[i * nsub + lane] = f;
                        u64 mk = __ballot(av > 0.0);
                        double v = f;
                        while (mk) {
                            const int c = __ffsll((unsigned long long)mk) - 1;
                            mk &= mk - 1ull;
                            const double ac = __shfl(av, c), pf = __shfl_xor(f, 1 << c);
                            if ((lane >> c) & 1) v = v + ac * pf;
                        }
                        f = v;
                    }
                    const double Z = __shfl(f, full);
                    if (lane == 0) {
                        Zs[kk] = Z;
                        logZ[kk] = (Z > 0.0) ? log(Z) : -INF;
                        if (!(Z > 0.0)) atomicOr(&ctl[5], 1);  // the whole frame is infeasible
                    }
                }
                __syncthreads();
                if (ctl[5] != 0) break;  // (uniform)
                for (int s = tid; s < p.nSample; s += NT) {
                    int *row = asg + (long long)s * M;
                    double l = lp[s];
                    for (int j = 0; j < n; j++) {
                        const int rootJ = clist[k + j], mJ = csize[rootJ], RJ = crows[rootJ], stJ = cstart[rootJ];
                        const double *hist = arena + j * (CS_WAVE_BYTES / 8);
                        const double prod = cs_walk(hist, hist + RJ * (1 << mJ), RJ, mJ, Zs[k + j], rowList + stJ, rowAct + stJ, rawRow,
                                                    wcol + j * 8, p.sampleBase + (u32)s, f0, f1, k0, k1, row);
                        l = l + (log(prod) - logZ[k + j]);
                    }
                    lp[s] = l;
                }
                __syncthreads();
                k += n;
                continue;
            }
            // ---- another cluster: the whole workgroup, with the forward sweep of kbest_perm.hip, then the walk -----------------------
            const int nsub = 1 << m;
            const unsigned full = (unsigned)nsub - 1u;
            // where the layers live changes no bit: a in LDS where it fits, the F layers too where they fit behind it
            const CsPlace where = cs_place(m, R, p.arenaBytes);
            double *a = where.aInArena ? arena : slice;
            double *hist = where.histInArena ? arena + where.histArenaOff : slice + aPart;
            if (wave == 0) {
                const u64 b0 = __ballot(lane < M && label[lane < M ? lane : 0] == root);
                const u64 b1 = __ballot(64 + lane < M && label[64 + lane < M ? 64 + lane : 0] == root);
                if (lane < m) ccol[lane] = cs_nth_bit128(b0, b1, lane);
            }
            __syncthreads();
            for (int i = tid; i < R * m; i += NT) {
                const int r = i / m, j = i - r * m;
                a[i] = cs_entry(Cg, NR, ccol[j], rawRow[rowList[st + r]], cond, colMin, mn);
            }
            for (int S = tid; S < nsub; S += NT) hist[S] = (S == 0) ? 1.0 : 0.0;
            __syncthreads();
            for (int r = tid; r < R; r += NT) {
                unsigned mk = 0;
                for (int j = 0; j < m; j++) mk |= (a[r * m + j] > 0.0) ? (1u << j) : 0u;
                locMask[r] = (unsigned short)mk;
            }
            __syncthreads();
            // forward sweep: hist[i] = F[i], i = 0 .. R - 1
            for (int i = 0; i + 1 < R; i++) {
                const double *ar = a + i * m;
                const unsigned mk = locMask[i];
                const double *Fi = hist + (long long)i * nsub;
                double *Fo = hist + (long long)(i + 1) * nsub;
                for (int S = tid; S < nsub; S += NT) Fo[S] = cs_layer_entry(Fi, ar, mk, (unsigned)S, i + 1);
                __syncthreads();
            }
            double Z = 0.0;
            if (R >= m) {  // Z = F[R][all], by the same expression  (R >= m >= 1)
                const double *ar = a + (R - 1) * m;
                const double *Fi = hist + (long long)(R - 1) * nsub;
                Z = Fi[full];
                unsigned cols = full & locMask[R - 1];
                while (cols) {
                    const int c = __ffs(cols) - 1;
                    cols &= cols - 1u;
                    Z = Z + ar[c] * Fi[full ^ (1u << c)];
                }
            }
            if (tid == 0) {
                logZ[k] = (Z > 0.0) ? log(Z) : -INF;
                if (!(Z > 0.0)) ctl[5] = 1;
            }
            if (!(Z > 0.0)) break;  // (uniform)
            const double lz = log(Z);
            for (int s = tid; s < p.nSample; s += NT) {
                const double prod = cs_walk(hist, a, R, m, Z, rowList + st, rowAct + st, rawRow, ccol, p.sampleBase + (u32)s, f0, f1, k0,
                                            k1, asg + (long long)s * M);
                lp[s] = lp[s] + (log(prod) - lz);
            }
            __syncthreads();
            k++;
        }
        __syncthreads();

        // ---- the frame: logPerm = sum of log Z_k in cluster order; one infeasible cluster leaves no draw -------------------------
        const bool bad = ctl[5] != 0;
        if (bad)
            for (int s = tid; s < p.nSample; s += NT) {  // (its owner: behind whatever it wrote for the clusters before)
                for (int c = 0; c < M; c++) asg[(long long)s * M + c] = -1;
                lp[s] = QNAN;
            }
        if (tid == 0) {
            double sum = 0.0;
            if (!bad)
                for (int j = 0; j < nClus; j++) sum = sum + logZ[j];
            if (p.logPerm) p.logPerm[b] = bad ? -INF : sum;
            if (p.info) p.info[b] = bad ? 0 : nClus;
        }
        __syncthreads();
    }
}

}  // namespace

#ifdef KB_CLUSTER_SAMPLE_PARTIAL
hipError_t launch_kbest_cluster_sample_partial(const ClusterSampleParams &p, int maxExact, const ClusterPlan &pl, int grid,
                                               hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int lds = cs_lds(p.maxRawRow, p.maxCol, pl.arena).total;
    if (lds != pl.lds || p.arenaBytes != pl.arena) return hipErrorInvalidValue;
    if (lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_cluster_sample_partial_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kbest_cluster_sample_partial_kernel, dim3(grid), dim3(pl.threads), lds, stream, p, maxExact);
    return hipGetLastError();
}
#else
hipError_t launch_kbest_cluster_sample(const ClusterSampleParams &p, const ClusterPlan &pl, int grid, hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int lds = cs_lds(p.maxRawRow, p.maxCol, pl.arena).total;  // (cluster_plan's pl.lds: the same layout)
    if (lds != pl.lds || p.arenaBytes != pl.arena) return hipErrorInvalidValue;
    if (lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_cluster_sample_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kbest_cluster_sample_kernel, dim3(grid), dim3(pl.threads), lds, stream, p);
    return hipGetLastError();
}
#endif

}  // namespace kb
