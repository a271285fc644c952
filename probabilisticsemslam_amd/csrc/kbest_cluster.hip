// kbest_cluster.hip -- clusterProb: the EXACT association probabilities of a frame by gated clusters, for frames of up to
// KBEST_CLUSTER_MAX_COLS measurements and KBEST_MAX_DIM_WIDE rows whose clusters have at most KBEST_CLUSTER_MAX_SIZE measurements.
// gfx950, fp64, plain HIP C++.  DESIGN.md section 11.
//
// a = toProbs(cost) >= 0, R x C, exactly the matrix kbest_perm.hip and kbest_lbp.hip work on (optional conditionCosts while loading,
// the exp and the expression of to_probs_kernel, the minimum of the WHOLE block).  Columns c and c' are adjacent when some row has a
// non-zero entry in both; a cluster is a connected component of columns with every row that has a non-zero entry in one of them.
// The permanent factorises over the clusters and so do the marginals: per cluster k (m_k columns, R_k rows) the recurrences of
// kbest_perm.hip on the sub-matrix give Z_k and w[r][c], and probs[c][min(r, nL)] += w[r][c] / Z_k; logPerm = sum_k log Z_k.
//
// One workgroup per frame at a time (the grid strides over the batch; a workgroup never waits for another one).
//   * prologue as kbest_perm.hip: conditionCosts while loading, the block minimum, the gate -- but a is never stored whole (up to
//     1 MB): per row the mask of its non-zero columns (two 64-bit words), and a cluster's entries are computed again from the cost
//     block (which stays in L2) when the cluster is worked on: the same expression, the same bits;
//   * labelling in LDS: label[c] = c, a thread per row takes the minimum label over its columns and writes it back with integer
//     atomicMin, until a sweep changes nothing: the lowest column of every component, whatever the order of the atomics;
//   * rows are sorted by cluster (stable: ascending row order inside a cluster), the columns of a cluster are compacted to its bit
//     positions in ascending column order;
//   * SMALL clusters (cl_small: at most 6 columns -- one subset per lane -- and layers of at most 4 KiB) are taken by single waves
//     side by side, without a workgroup barrier: the layer lives in one register per lane, its neighbours S ^ {c} come by
//     shuffles, the history of the forward sweep in the wave's own 4 KiB of LDS, the marginal sums by one fixed DPP butterfly;
//   * the other clusters by the whole workgroup, one after another, with the sweeps of kbest_perm.hip: perm_threads(m_k) threads
//     accumulate, their sums are added over the wave (the same butterfly) and over the waves in ascending order; layers in LDS
//     where they fit, else in the workgroup's slot of a work space in HBM (the same instructions on either).
// Which tier takes a cluster and how its sums are shaped is a function of m_k and R_k alone and there are no floating-point
// atomics: a frame's result does not depend on the batch it travels in, on the launch's bounds or on the caps, bit for bit.
//   * a cluster of more than 16 columns: info = -2; layers (R_k + 2) 2^m_k 8 bytes beyond the slot: info = -3; zeros, logPerm NaN;
//   * some Z_k == 0 (a column without a finite entry, fewer usable rows than columns in a cluster): zeros, logPerm = -inf, info 0.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_wave_sum.h"

namespace kb {

namespace {

constexpr double CL_GATE = 42.0;     // assignment.cpp:9
constexpr int CL_MAX_COLS = 128;     // KBEST_CLUSTER_MAX_COLS: two mask words per row
constexpr int CL_MAX_SIZE = 16;      // KBEST_CLUSTER_MAX_SIZE
constexpr int CL_WAVE_BYTES = 4096;  // LDS of one wave of the small tier: R 2^m history + R m entries
constexpr int CL_SPT = 4;            // subsets per accumulating thread, as PM_SPT of kbest_perm.hip

// threads that accumulate the marginals of a cluster of m columns in the workgroup tier: perm_threads of kbest_perm.hip, but 512
// at the most -- with both tiers in one kernel 1 024 threads (128 VGPRs) spill in the sweeps, 512 (155 VGPRs) do not.  Part of the
// result's bits: the order of the sums follows from it.
__host__ __device__ inline int cl_threads(int m)
{
    const int t = (1 << m) / CL_SPT;
    return t < 64 ? 64 : t > 512 ? 512 : t;
}

// the tier of a cluster: a function of its own columns and rows only
__host__ __device__ inline bool cl_small(int m, int R) { return m <= 6 && (R * (1 << m) + R * m) * 8 <= CL_WAVE_BYTES; }

// the j-th set bit (ascending) of a 128-bit mask that has more than j bits
__device__ __forceinline__ int nth_bit128(u64 lo, u64 hi, int j)
{
    for (int t = 0; t < j; t++) {
        if (lo) lo &= lo - 1ull;
        else hi &= hi - 1ull;
    }
    return lo ? __ffsll((unsigned long long)lo) - 1 : 64 + __ffsll((unsigned long long)hi) - 1;
}

struct ClLds {  // byte offsets into the dynamic LDS
    int red, colMin, waveMin, ctl, logZ, label, csize, crows, cstart, clist, ccol, rawRow, flag, act, rowRoot, rowList, locMask,
        maskLo, maskHi, arena, total;
};

__host__ __device__ inline ClLds cl_lds(int maxRawRow, int maxCol, int arenaBytes)
{
    ClLds l;
    int o = 0;
    l.red = o;     o += 2 * 16 * 16 * 8;  // [2][wave][column]
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
    l.flag = o;    o += rows2;            // u16: row kept / row active
    l.act = o;     o += rows2;            // u16: kept index of every active (non-zero) row
    l.rowRoot = o; o += rows2;            // u16: the root of every active row
    l.rowList = o; o += rows2;            // u16: kept indices sorted by cluster
    l.locMask = o; o += rows2;            // u16: non-zero columns of the rows of the cluster the workgroup works on
    l.maskLo = o;  o += maxRawRow * 8;    // u64: non-zero columns 0..63 of every kept row
    l.maskHi = o;  o += maxRawRow * 8;    // ... and 64..127
    o = (o + 15) & ~15;
    l.arena = o;   o += arenaBytes;       // the small tier: CL_WAVE_BYTES per wave; the workgroup tier: G layers, a, F layers
    l.total = (o + 15) & ~15;
    return l;
}

// one entry of a: conditionCosts (assignment.cpp:490-494) and toProbs (:536-540) on the raw cost, as to_probs_kernel has it
__device__ __forceinline__ double cl_entry(const double *Cg, int NR, int c, int raw, bool condition, const double *colMin, double mn)
{
    double x = Cg[(long long)c * NR + raw];
    if (condition) x = (x <= colMin[c] + CL_GATE) ? (x - colMin[c]) : d_inf();
    return (mn + CL_GATE > x) ? exp(mn - x) : 0.0;
}

// ... and whether it is non-zero: the gate alone (exp of more than -42 is positive)
__device__ __forceinline__ bool cl_nonzero(const double *Cg, int NR, int c, int raw, bool condition, const double *colMin, double mn)
{
    double x = Cg[(long long)c * NR + raw];
    if (condition) x = (x <= colMin[c] + CL_GATE) ? (x - colMin[c]) : d_inf();
    return mn + CL_GATE > x;
}

// The partial mode hands one open cluster out: its (nLk + m) x m column-major sub-block -- the cluster's
// rows in ascending raw order (the nLk landmark rows first), then all-+inf rows up to nLk + m; its columns ascending; the value
// cl_entry forms before the exp, +inf where cl_nonzero is false -- and its landmark rows in the caller's numbering.  Every thread
// of the workgroup calls it; eCol (LDS) takes the cluster's columns.  Kept out of line: the sweeps' registers are not its.
__device__ __noinline__ void cl_emit_open(const double *Cg, int NR, int M, bool cond, const double *colMin, double mn, const int *label,
                                          int root, const unsigned short *rawRow, const unsigned short *rows, int R, int m, int nLk,
                                          int *eCol, double *sub, int *rowOut)
{
    const int tid = threadIdx.x, NT = blockDim.x;
    for (int c = tid; c < M; c += NT)
        if (label[c] == root) {
            int rank = 0;
            for (int j = 0; j < c; j++) rank += (label[j] == root) ? 1 : 0;
            eCol[rank] = c;
        }
    __syncthreads();
    const int nr = nLk + m;
    for (int i = tid; i < nr * m; i += NT) {
        const int j = i / nr, r = i - j * nr;
        double v = d_inf();
        if (r < R) {
            const int c = eCol[j];
            double x = Cg[(long long)c * NR + rawRow[rows[r]]];
            if (cond) x = (x <= colMin[c] + CL_GATE) ? (x - colMin[c]) : d_inf();
            v = (mn + CL_GATE > x) ? x : d_inf();
        }
        sub[i] = v;
    }
    for (int r = tid; r < nLk; r += NT) rowOut[r] = rawRow[rows[r]];
    __syncthreads();
}

// PARTIAL = false: every existing entry.  PARTIAL = true (kbest_clustered_partial_batch_f64_dev): a cluster of more than
// q.maxExact columns, or whose layers exceed the slot, is OPEN: it does not refuse the frame, its columns stay 0.0 and its
// sub-problem is handed out; every other cluster goes through the same tiers, the same sums, the same bits.
struct ClusterNoOpen {};  // the plain kernel's second argument: nothing

template <bool PARTIAL>
__global__ void __launch_bounds__(512)
kbest_cluster_kernel(ClusterParams p, [[maybe_unused]] std::conditional_t<PARTIAL, ClusterOpenParams, ClusterNoOpen> q)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NWV = NT >> 6;
    const ClLds L = cl_lds(p.maxRawRow, p.maxCol, p.arenaBytes);
    double *red = reinterpret_cast<double *>(smem + L.red);
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
    unsigned short *act = reinterpret_cast<unsigned short *>(smem + L.act);
    unsigned short *rowRoot = reinterpret_cast<unsigned short *>(smem + L.rowRoot);
    unsigned short *rowList = reinterpret_cast<unsigned short *>(smem + L.rowList);
    unsigned short *locMask = reinterpret_cast<unsigned short *>(smem + L.locMask);
    u64 *maskLo = reinterpret_cast<u64 *>(smem + L.maskLo);
    u64 *maskHi = reinterpret_cast<u64 *>(smem + L.maskHi);
    double *arena = reinterpret_cast<double *>(smem + L.arena);
    double *slice = p.work + (long long)blockIdx.x * p.slotStride;  // this workgroup's part of the work space
    const long long aPart = (long long)p.maxRawRow * CL_MAX_SIZE;   // ... its first doubles: a of a cluster; then the layers
    const double INF = d_inf();
    const bool cond = p.condition != 0;

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M;
        double *probOut = p.probs + p.probOff[b];
        const double *Cg = p.cost + p.costOff[b];
        // (uniform over the workgroup) a frame beyond what the launch was sized for: info = -1 and nothing else is touched
        if (M < 1 || M > p.maxCol || M > CL_MAX_COLS || nLo < 0 || NR > p.maxRawRow) {
            if (tid == 0 && p.info) p.info[b] = -1;
            if constexpr (PARTIAL)
                if (tid == 0) q.nOpen[b] = 0;
            continue;
        }
        for (int i = tid; i < M * (nLo + 1); i += NT) probOut[i] = 0.0;  // (rows conditionCosts drops, zero rows: exactly 0.0)

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
                for (int c = 0; c < M; c++) good = good | (Cg[(long long)c * NR + r] <= colMin[c] + CL_GATE);
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
                if (cond) x = (x <= colMin[c] + CL_GATE) ? (x - colMin[c]) : INF;  // (:490-494)
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
                const bool nz = cl_nonzero(Cg, NR, c, raw, cond, colMin, mn);
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
                int m = CL_MAX_COLS;
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
            [[maybe_unused]] int nOpenT = 0;
            for (int c = 0; c < M; c++)
                if (label[c] == c) {
                    const int m = csize[c], R = crows[c];
                    clist[n++] = c;
                    cstart[c] = at;
                    at += R;
                    if (m > maxC) maxC = m;
                    if constexpr (PARTIAL) {  // answered clusters from the front of clist, open ones from its back: both in label order
                        if (m > q.maxExact || ((long long)(R + 2) << m) * 8 > p.slotBytes) {
                            n--;
                            clist[M - 1 - nOpenT++] = c;
                        }
                    } else {
                        if (m > CL_MAX_SIZE) refuse = -2;
                        else if (refuse == 0 && ((long long)(R + 2) << m) * 8 > p.slotBytes) refuse = -3;
                    }
                }
            ctl[2] = n;
            ctl[3] = maxC;
            ctl[4] = refuse;
            if constexpr (PARTIAL) ctl[6] = nOpenT;
        }
        __syncthreads();
        const int nClus = ctl[2], refuse = ctl[4];
        if (tid == 0 && p.maxCluster) p.maxCluster[b] = ctl[3];
        if (p.label)
            for (int c = tid; c < p.labelStride; c += NT) p.label[(long long)b * p.labelStride + c] = c < M ? label[c] : -1;
        if (refuse != 0) {  // (uniform) the zeros stay
            if (tid == 0) {
                if (p.info) p.info[b] = refuse;
                if (p.logPerm) p.logPerm[b] = __longlong_as_double(0x7ff8000000000000LL);
            }
            __syncthreads();
            continue;
        }
        for (int i = tid; i < Ra; i += NT) {
            const int root = rowRoot[i];
            int rank = 0;
            for (int j = 0; j < i; j++) rank += (rowRoot[j] == root) ? 1 : 0;
            rowList[cstart[root] + rank] = act[i];
        }
        __syncthreads();
        [[maybe_unused]] int nOpen = 0;
        if constexpr (PARTIAL) {
            // ---- the open clusters, in label order: their landmark rows counted, their places in the outputs, then handed out ---------
            nOpen = ctl[6];
            int *eNL = reinterpret_cast<int *>(red), *eRowOff = eNL + CL_MAX_COLS, *eCol = eRowOff + CL_MAX_COLS;  // (red: free until
            long long *eSubOff = reinterpret_cast<long long *>(eCol + CL_MAX_COLS);                               //  the sweeps)
            for (int j = tid; j < nOpen; j += NT) {
                const int root = clist[M - 1 - j], R = crows[root], st = cstart[root];
                int n = 0;
                for (int r = 0; r < R; r++) n += (rawRow[rowList[st + r]] < nLo) ? 1 : 0;
                eNL[j] = n;
            }
            __syncthreads();
            if (tid == 0) {
                int rowAt = 0, layout = 0;
                long long subAt = 0;
                for (int j = 0; j < nOpen; j++) {
                    const int root = clist[M - 1 - j], m = csize[root];
                    if (crows[root] - eNL[j] > m) layout = -2;  // more rows >= nL than columns: not the reference's layout
                    eRowOff[j] = rowAt;
                    eSubOff[j] = subAt;
                    rowAt += eNL[j];
                    subAt += (long long)(eNL[j] + m) * m;
                }
                ctl[4] = layout;
            }
            __syncthreads();
            if (ctl[4] != 0) {  // (uniform) refused as a whole: zeros, nothing handed out
                if (tid == 0) {
                    if (p.info) p.info[b] = ctl[4];
                    if (p.logPerm) p.logPerm[b] = __longlong_as_double(0x7ff8000000000000LL);
                    q.nOpen[b] = 0;
                }
                __syncthreads();
                continue;
            }
            for (int j = 0; j < nOpen; j++) {  // (uniform)
                const int root = clist[M - 1 - j], m = csize[root];
                if (tid == 0) {
                    int *d = q.openDesc + ((long long)b * q.descStride + j) * 4;
                    d[0] = root;
                    d[1] = m;
                    d[2] = eNL[j];
                    d[3] = crows[root];
                }
                cl_emit_open(Cg, NR, M, cond, colMin, mn, label, root, rawRow, rowList + cstart[root], crows[root], m, eNL[j], eCol,
                             q.sub + p.costOff[b] + eSubOff[j], q.openRows + (long long)b * q.rowStride + eRowOff[j]);
            }
        }

        // ---- the small clusters: one wave each, side by side, no workgroup barrier ------------------------------------------------
        for (int k = wave; k < nClus; k += NWV) {
            const int root = clist[k], m = csize[root], R = crows[root], st = cstart[root];
            if (!cl_small(m, R)) continue;  // (uniform over the wave)
            const int nsub = 1 << m, full = nsub - 1;
            const u64 b0 = __ballot(lane < M && label[lane < M ? lane : 0] == root);
            const u64 b1 = __ballot(64 + lane < M && label[64 + lane < M ? 64 + lane : 0] == root);
            const int colj = lane < m ? nth_bit128(b0, b1, lane) : 0;
            const bool inS = lane < nsub;
            double *hist = arena + wave * (CL_WAVE_BYTES / 8);  // [R][nsub]: lane S writes and reads its own entries only
            double *aSt = hist + R * nsub;                      // [R][m]: lane j likewise
            double f = lane == 0 ? 1.0 : 0.0;                   // F[i][S] in lane S
            for (int i = 0; i < R; i++) {
                const int raw = rawRow[rowList[st + i]];
                double av = 0.0;
                if (lane < m) {
                    av = cl_entry(Cg, NR, colj, raw, cond, colMin, mn);
                    aSt[i * m + lane] = av;
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
            if (lane == 0) logZ[k] = (Z > 0.0) ? log(Z) : -INF;
            if (!(Z > 0.0)) {  // (uniform over the wave) the whole frame is infeasible
                if (lane == 0) atomicOr(&ctl[5], 1);
                continue;
            }
            double g = lane == 0 ? 1.0 : 0.0;  // G[r+1][S] in lane S
            double missAcc = 0.0;              // lane j: slot nL of the cluster's column j, rows added in descending order
            for (int r = R - 1; r >= 0; r--) {
                const int raw = rawRow[rowList[st + r]];
                const double av = lane < m ? aSt[r * m + lane] : 0.0;
                const double fr = inS ? hist[r * nsub + lane] : 0.0;
                const u64 mk0 = __ballot(av > 0.0);
                for (u64 mk = mk0; mk; mk &= mk - 1ull) {
                    const int c = __ffsll((unsigned long long)mk) - 1;
                    const double gv = __shfl(g, (full ^ lane ^ (1 << c)) & 63);
                    const double term = (inS && !((lane >> c) & 1)) ? fr * gv : 0.0;
                    const double s = readlane_f64(wave_sum63_f64(term), 63);
                    if (lane == c) {
                        const double wv = av * s;
                        if (raw < nLo) probOut[colj * (nLo + 1) + raw] = wv / Z;  // scatter back to the caller's numbering (:68-74)
                        else missAcc = missAcc + wv;
                    }
                }
                double v = g;
                for (u64 mk = mk0; mk; mk &= mk - 1ull) {
                    const int c = __ffsll((unsigned long long)mk) - 1;
                    const double ac = __shfl(av, c), pg = __shfl_xor(g, 1 << c);
                    if ((lane >> c) & 1) v = v + ac * pg;
                }
                g = v;
            }
            if (lane < m) probOut[colj * (nLo + 1) + nLo] = missAcc / Z;
        }
        __syncthreads();

        // ---- the other clusters: the whole workgroup, one after another, with the sweeps of kbest_perm.hip -----------------------
        for (int k = 0; k < nClus; k++) {
            const int root = clist[k], m = csize[root], R = crows[root], st = cstart[root];
            if (cl_small(m, R)) continue;  // (uniform)
            const int nsub = 1 << m;
            const unsigned full = (unsigned)nsub - 1u;
            // where the layers live changes no bit: G and a in LDS where they fit, the F layers too where they fit beside them
            const long long gaBytes = (2ll * nsub + (long long)R * m) * 8, allBytes = gaBytes + (long long)R * nsub * 8;
            double *g, *a, *hist;
            if (gaBytes <= p.arenaBytes) {
                g = arena;
                a = arena + 2 * nsub;
                hist = (allBytes <= p.arenaBytes) ? a + R * m : slice + aPart;
            } else {
                a = slice;
                g = slice + aPart;
                hist = g + 2ll * nsub;
            }
            if (wave == 0) {
                const u64 b0 = __ballot(lane < M && label[lane < M ? lane : 0] == root);
                const u64 b1 = __ballot(64 + lane < M && label[64 + lane < M ? 64 + lane : 0] == root);
                if (lane < m) ccol[lane] = nth_bit128(b0, b1, lane);
            }
            __syncthreads();
            for (int i = tid; i < R * m; i += NT) {
                const int r = i / m, j = i - r * m;
                a[i] = cl_entry(Cg, NR, ccol[j], rawRow[rowList[st + r]], cond, colMin, mn);
            }
            for (int S = tid; S < nsub; S += NT) {
                hist[S] = (S == 0) ? 1.0 : 0.0;
                g[S] = (S == 0) ? 1.0 : 0.0;  // G[R]
            }
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
                }
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
            if (!(Z > 0.0)) {  // (uniform)
                __syncthreads();
                continue;
            }
            // backward sweep with the marginals
            const int nt = cl_threads(m) < NT ? cl_threads(m) : NT;  // (NT >= cl_threads(m): the launch is sized by maxCol >= m)
            double missAcc = 0.0;  // thread j: slot nL of the cluster's column j, rows added in descending order
            int pg = 0;
            for (int r = R - 1; r >= 0; r--) {
                const double *ar = a + r * m;
                const unsigned mk = locMask[r];
                const double *Fr = hist + (long long)r * nsub;
                const double *Gc = g + (long long)pg * nsub;  // G[r+1]
                double *Gn = g + (long long)(pg ^ 1) * nsub;  // G[r]
                double *redP = red + (r & 1) * 256;
                if (tid < nt) {
                    double acc[16];
#pragma unroll
                    for (int c = 0; c < 16; c++) acc[c] = 0.0;
                    for (int S0 = tid; S0 < nsub; S0 += CL_SPT * nt) {  // (the loads of a batch first: F[r] may live in HBM)
                        double fv[CL_SPT];
#pragma unroll
                        for (int j = 0; j < CL_SPT; j++) fv[j] = (S0 + j * nt < nsub) ? Fr[S0 + j * nt] : 0.0;
#pragma unroll
                        for (int j = 0; j < CL_SPT; j++) {
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
                    const int left = R - r;  // rows r .. R-1
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
                if (tid < m && ((mk >> tid) & 1u)) {
                    double s = redP[tid];
                    for (int w = 1; w < (nt >> 6); w++) s = s + redP[w * 16 + tid];
                    const double wv = ar[tid] * s;
                    const int raw = rawRow[rowList[st + r]];
                    if (raw < nLo) probOut[ccol[tid] * (nLo + 1) + raw] = wv / Z;  // scatter back to the caller's numbering (:68-74)
                    else missAcc = missAcc + wv;
                }
                pg ^= 1;
            }
            if (tid < m) probOut[ccol[tid] * (nLo + 1) + nLo] = missAcc / Z;
            __syncthreads();
        }
        __syncthreads();

        // ---- the frame: logPerm = sum of log Z_k in cluster order; one infeasible cluster makes the whole frame zeros --------------
        const bool bad = ctl[5] != 0;
        if (bad)
            for (int i = tid; i < M * (nLo + 1); i += NT) probOut[i] = 0.0;
        if (tid == 0) {
            double lp = 0.0;
            for (int k = 0; k < nClus; k++) lp = lp + logZ[k];
            if (p.logPerm) p.logPerm[b] = bad ? -INF : lp;
            if constexpr (PARTIAL) {
                if (p.info) p.info[b] = bad ? 0 : nClus + nOpen;
                q.nOpen[b] = bad ? 0 : nOpen;
            } else {
                if (p.info) p.info[b] = bad ? 0 : nClus;
            }
        }
        __syncthreads();
    }
}

}  // namespace

ClusterPlan cluster_plan(int maxRawRow, int maxCol, int ldsLimit, size_t slotCap)
{
    ClusterPlan pl;
    const int mc = maxCol < CL_MAX_SIZE ? maxCol : CL_MAX_SIZE;
    pl.threads = cl_threads(mc);
    // the arena: the small tier's CL_WAVE_BYTES per wave at least; all layers of the largest cluster the bounds allow where that
    // stays within 64 KiB (two workgroups a CU)
    const long long all = (((long long)(maxRawRow + 2) << mc) + (long long)maxRawRow * mc) * 8;
    long long arena = (pl.threads / 64) * CL_WAVE_BYTES;
    const long long hi = 64 << 10;
    if (all > arena) arena = all < hi ? all : (hi > arena ? hi : arena);
    long long fixed = cl_lds(maxRawRow, maxCol, 0).total;
    if (fixed + arena > ldsLimit) arena = ldsLimit - fixed;
    arena &= ~15ll;
    if (arena < (pl.threads / 64) * CL_WAVE_BYTES) arena = -1;  // (a device without the LDS for the small tier: no plan)
    pl.arena = (int)arena;
    pl.lds = arena < 0 ? -1 : cl_lds(maxRawRow, maxCol, pl.arena).total;
    unsigned long long layers = ((unsigned long long)(maxRawRow + 2) << mc) * 8ull;
    if (layers > slotCap) layers = slotCap;
    layers = (layers + 7ull) & ~7ull;
    pl.slotBytes = (long long)layers;
    pl.slotDoubles = (long long)maxRawRow * CL_MAX_SIZE + (long long)(layers / 8);
    return pl;
}

hipError_t launch_kbest_cluster(const ClusterParams &p, const ClusterPlan &pl, int grid, hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (pl.lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_cluster_kernel<false>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(pl.lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kbest_cluster_kernel<false>, dim3(grid), dim3(pl.threads), pl.lds, stream, p, ClusterNoOpen{});
    return hipGetLastError();
}

hipError_t launch_kbest_cluster_partial(const ClusterParams &p, const ClusterOpenParams &q, const ClusterPlan &pl, int grid,
                                        hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (pl.lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_cluster_kernel<true>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, pl.lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(pl.lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kbest_cluster_kernel<true>, dim3(grid), dim3(pl.threads), pl.lds, stream, p, q);
    return hipGetLastError();
}

}  // namespace kb
