// kbest_frontier_sample.hip -- joint associations DRAWN from the exact posterior of a sparse cluster of up to
// KBEST_FRONTIER_MAX_COLS = 64 measurements whose frontier width is at most KBEST_FRONTIER_MAX_WIDTH = 16: the plan and the forward
// sweep of kbest_frontier.hip, then one backward walk per draw over the layers that sweep keeps.  One workgroup per cluster, one
// launch per pack of clusters.  gfx950, fp64, plain HIP C++.  DESIGN.md section 18.
// Two entry points, one walk (frontier_sample_walk<Source>): frontier_sample_kernel takes its clusters from a kernel-argument pack,
// frontier_sample_list_kernel from the list kbest_hybrid.hip gathers and kbest_hybrid_sample.hip completes on the device, ONE launch
// for all of them.
//
// Input, scaling, plan and forward layers are kbest_frontier.hip's, restated expression for expression (that file keeps its own
// lines and with them its code objects): the (nL_k + m_k) x m_k column-major sub-block, a'[r][c] = exp(colMin_c - x[r][c]), the
// greedy row order, Phi_i / Psi_i / closing_i / new_i, F_0 = {empty: 1},
//     F_{i+1}[S] = [T & new = 0] F_i[T] + sum_{c in T & N_r, (T \ c) & new = 0, c ascending} a'[r][c] F_i[T \ c],   T = S | closing_i
// Z' = F_R[empty]; logZ, info (1 / 0 / -3 / -4 / -5, the range check and the count of that file included) and width are that tier's,
// bit for bit -- the slot is counted with the two buffers of its backward sweep although nothing is swept backward here, so that a
// cluster is refused here exactly when it is refused there.
//
// The walk: thread t owns FS_DPT draws of a round of FS_THREADS * FS_DPT; all threads go through the steps of the plan together,
// from the last to the first, and wave 0 stages a step (its description, its a', its masks, its row key) in LDS once per round for
// the whole workgroup.  A draw starts at S = empty in Phi_R; at step i with row r: T = S | closing_i in Psi_i, tot = F_{i+1}[S],
// Tt = u tot, acc = 0;
//     T & new_i == 0: acc = F_i[T]; Tt < acc: the row takes nothing, S = T in Phi_i
//     else the columns c of T & N_r in ascending order with (T \ c) & new_i == 0: acc += a'[r][c] F_i[T \ c]; the first c with
//     Tt < acc is taken (if rounding leaves none: the last c whose term was > 0), S = T \ c in Phi_i
// a'[r][c] is the sweep's expression, so the terms are the sweep's bits.  The uniform: Philox4x32-10, key (seed low, seed high),
// counter (sampleBase + s, 0x80000000 | (q >> 1), frameKey low, frameKey high), words 0, 1 for an even q and 2, 3 for an odd one,
// q = rowKey[row of the sub-block]: bit 31 of the second word keeps these uniforms apart from kbest_cluster_sample.hip's.
// Out: assignLocal[s][c] = the row of the sub-block column c takes; logTerm[s] = sum_c (colMin_c - x[r_c][c]) - log Z', the columns
// in ascending order, no log of a product.  info 0 (no complete assignment): assignLocal -1, logTerm NaN; a refusal (-3, -4, -5):
// neither is touched.
// No workgroup waits for another (no grid barrier, no flag), no floating-point atomics, no sum over threads: a cluster's outputs
// are a function of (cluster, row keys, seed, frame key, draw index) alone, anywhere in a batch and under any cap.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_cluster_sample.h"

namespace kb {

namespace {

constexpr int FS_THREADS = KB_FRONTIER_THREADS;
constexpr int FS_W = KB_FRONTIER_MAX_WIDTH;
constexpr int FS_ROWS = KB_FRONTIER_MAX_ROWS;
constexpr int FS_DPT = 4;  // draws a thread walks side by side: a step is staged once for FS_THREADS * FS_DPT draws

// ---- kbest_frontier.hip's plan step, helpers and shared block, restated: that file stays as it is ------------------------------------
struct FsStep {        // KB_FRONTIER_STEP_DOUBLES * 8 bytes (FrontierStep)
    long long off;     // F_i, in doubles from the slot
    int row;           // the counting row it takes
    int nPsi, nPhi, nNext;
    int pad;
    signed char col[FS_W], posPhi[FS_W], posNext[FS_W];  // per bit of Psi_i
};
static_assert(sizeof(FsStep) == KB_FRONTIER_STEP_DOUBLES * 8, "FsStep");

// the bits of v at the places of mask, packed / the low bits of v spread to the places of mask (mask uniform, at most 16 bits)
__device__ __forceinline__ unsigned fs_pack_bits(unsigned v, unsigned mask)
{
    unsigned r = 0, k = 1;
    while (mask) {
        const unsigned b = mask & (0u - mask);
        r |= (v & b) ? k : 0u;
        k <<= 1;
        mask ^= b;
    }
    return r;
}
__device__ __forceinline__ unsigned fs_spread_bits(unsigned v, unsigned mask)
{
    unsigned r = 0;
    while (mask) {
        const unsigned b = mask & (0u - mask);
        r |= (v & 1u) ? b : 0u;
        v >>= 1;
        mask ^= b;
    }
    return r;
}

struct FsShared {
    u64 mask[FS_ROWS];          // N_r of the counting rows
    int rowIdx[FS_ROWS];        // their rows in the sub-block
    unsigned char done[FS_ROWS];
    double colMin[KB_FRONTIER_MAX_COLS];
    double aval[FS_W];          // a'[r][column of bit j], 0 outside N_r
    u64 seen, open, last;
    long long off;
    double sumCol;
    unsigned key[FS_THREADS / 64];
    unsigned nrM, newM, closeM;  // bits of Psi_i: in N_r / not in Phi_i / not in Phi_{i+1}
    int R, W, emptyCol;
    int lost;                    // a finite entry whose a' is 0
    int subRow;                  // the walk: the step's row in the sub-block ...
    unsigned q;                  // ... and its key
    FsStep st;
};

// the step's description from the plan, its a' (unit: 1 for every non-zero one) and its masks: wave 0; a barrier follows.
// rowKey: the walk's (or nullptr)
__device__ __forceinline__ void fs_load_step(FsShared &sh, const FsStep *plan, int i, const double *x, int nr, int tid, const int *rowKey,
                                             bool unit)
{
    if (tid < 64) {
        const FsStep &g = plan[i];
        const int nPsi = g.nPsi;
        bool inN = false, isNew = false, closes = false;
        if (tid < nPsi) {
            const int c = g.col[tid], pp = g.posPhi[tid], pn = g.posNext[tid];
            sh.st.col[tid] = (signed char)c;
            sh.st.posPhi[tid] = (signed char)pp;
            sh.st.posNext[tid] = (signed char)pn;
            inN = (sh.mask[g.row] >> c) & 1ull;
            isNew = pp < 0;
            closes = pn < 0;
            sh.aval[tid] = !inN ? 0.0 : unit ? 1.0 : exp(sh.colMin[c] - x[(long long)c * nr + sh.rowIdx[g.row]]);
        }
        const u64 bN = __ballot(inN), bNew = __ballot(isNew), bClose = __ballot(closes);
        if (tid == 0) {
            sh.st.off = g.off;
            sh.st.row = g.row;
            sh.st.nPsi = nPsi;
            sh.st.nPhi = g.nPhi;
            sh.st.nNext = g.nNext;
            sh.nrM = (unsigned)bN;
            sh.newM = (unsigned)bNew;
            sh.closeM = (unsigned)bClose;
            const int sr = sh.rowIdx[g.row];
            sh.subRow = sr;
            sh.q = rowKey ? (unsigned)rowKey[sr] : 0u;
        }
    }
}

// F_0 .. F_R of a planned cluster into its slot; unit: every non-zero a' is 1, and F_R[empty] counts the complete assignments
__device__ __forceinline__ void fs_forward_sweep(FsShared &sh, const FsStep *plan, const double *x, int nr, int R, double *slot,
                                                 long long offR, int tid, bool unit)
{
    if (tid == 0) slot[0] = 1.0;
    __syncthreads();
    for (int i = 0; i < R; i++) {
        fs_load_step(sh, plan, i, x, nr, tid, nullptr, unit);
        __syncthreads();
        const unsigned psiM = (1u << sh.st.nPsi) - 1u, newM = sh.newM, closeM = sh.closeM, nrM = sh.nrM;
        const unsigned keepM = psiM & ~closeM, phiM = psiM & ~newM;
        const double *Fi = slot + sh.st.off;
        double *Fn = slot + (i + 1 < R ? plan[i + 1].off : offR);
        const int nS = 1 << sh.st.nNext;
        for (int S = tid; S < nS; S += FS_THREADS) {
            const unsigned T = fs_spread_bits((unsigned)S, keepM) | closeM;
            const unsigned nw = T & newM;
            const unsigned base = fs_pack_bits(T, phiM);
            double val = 0.0;
            if (nw == 0) {
                val = Fi[base];
                unsigned cols = T & nrM;
                while (cols) {
                    const int j = __ffs(cols) - 1;
                    cols &= cols - 1u;
                    val = val + sh.aval[j] * Fi[base ^ (1u << sh.st.posPhi[j])];
                }
            } else if ((nw & (nw - 1u)) == 0) {  // one new column: the row takes it
                val = sh.aval[__ffs(nw) - 1] * Fi[base];
            }
            Fn[S] = val;
        }
        __syncthreads();
    }
}

// Where the clusters of a launch come from: the kernel-argument pack of kbest_frontier_sample_f64_dev, or the list that
// kbest_hybrid.hip gathers and kbest_hybrid_sample.hip completes in HBM, with its count word.  The walk below is the same code for both.
struct FsPackSource {
    const FrontierSamplePack &p;
    __device__ __forceinline__ int n() const { return p.n; }
    __device__ __forceinline__ bool sent(int) const { return true; }
    __device__ __forceinline__ int m(int k) const { return p.c[k].m; }
    __device__ __forceinline__ int nL(int k) const { return p.c[k].nL; }
    __device__ __forceinline__ long long subOff(int k) const { return p.c[k].subOff; }
    __device__ __forceinline__ long long rowKeyOff(int k) const { return p.c[k].rowKeyOff; }
    __device__ __forceinline__ long long asgOff(int k) const { return p.c[k].asgOff; }
    __device__ __forceinline__ long long ltOff(int k) const { return p.c[k].ltOff; }
    __device__ __forceinline__ u64 frameKey(int k) const { return p.c[k].frameKey; }
    __device__ __forceinline__ int idx(int k) const { return p.base + k; }
};
struct FsListSource {
    const HybridItem *list;
    const HybridKeyItem *keys;
    const int *count;
    __device__ __forceinline__ int n() const { return *count; }
    __device__ __forceinline__ bool sent(int k) const { return keys[k].sent != 0; }
    __device__ __forceinline__ int m(int k) const { return list[k].m; }
    __device__ __forceinline__ int nL(int k) const { return list[k].nL; }
    __device__ __forceinline__ long long subOff(int k) const { return list[k].subOff; }
    __device__ __forceinline__ long long rowKeyOff(int k) const { return keys[k].rowKeyOff; }
    __device__ __forceinline__ long long asgOff(int k) const { return keys[k].asgOff; }
    __device__ __forceinline__ long long ltOff(int k) const { return keys[k].ltOff; }
    __device__ __forceinline__ u64 frameKey(int k) const { return keys[k].frameKey; }
    __device__ __forceinline__ int idx(int k) const { return k; }
};

template <class Source>
__device__ __forceinline__ void frontier_sample_walk(FsShared &sh, const Source &src, const double *sub, const int *rowKeys, int nSample,
                                                     u64 seed, u32 sampleBase, int *assignLocal, double *logTerm, double *logZ,
                                                     int *info, int *width, const FrontierWork &wk)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *slot = wk.layers + (long long)blockIdx.x * wk.slotDoubles;
    FsStep *plan = reinterpret_cast<FsStep *>(wk.plan + (long long)blockIdx.x * wk.planDoubles);
    const double INF = d_inf();
    const double QNAN = __builtin_nan("");
    const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32);
    const int n = src.n();
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        if (!src.sent(k)) continue;  // (uniform)
        const int m = src.m(k), nL = src.nL(k), nr = nL + m, idx = src.idx(k);
        const double *x = sub + src.subOff(k);
        const int *rowKey = rowKeys + src.rowKeyOff(k);
        int *asg = assignLocal + src.asgOff(k);
        double *lt = logTerm + src.ltOff(k);
        __syncthreads();  // (the previous cluster is done with the shared arrays)
        if ((long long)nr * KB_FRONTIER_STEP_DOUBLES > wk.planDoubles || nr > FS_ROWS || m > KB_FRONTIER_MAX_COLS) {
            if (tid == 0 && info) info[idx] = -3;  // (the host entry never lets this happen)
            continue;
        }
        // ---- setup: column minima, the rows that count, the row masks ------------------------------------------------------
        if (tid < m) {
            double mn = INF;
            for (int r = 0; r < nr; r++) mn = min_keep(mn, x[(long long)tid * nr + r]);
            sh.colMin[tid] = mn;
        }
        if (tid == 0) sh.lost = 0;
        __syncthreads();
        for (int r = tid; r < nr; r += FS_THREADS) {
            u64 mk = 0;
            bool any = false;
            for (int c = 0; c < m; c++) {
                const double e = x[(long long)c * nr + r];
                any = any | (e < INF);
                if (e < INF && exp(sh.colMin[c] - e) > 0.0) mk |= 1ull << c;
                else if (e < INF) sh.lost = 1;
            }
            sh.mask[r] = mk;
            sh.done[r] = any ? 1 : 0;  // (until the rows are counted below)
        }
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int c = 0; c < m; c++) s = s + (sh.colMin[c] < INF ? sh.colMin[c] : 0.0);
            sh.sumCol = s;
            int n = 0;
            for (int r = 0; r < nr; r++)
                if (sh.done[r]) {
                    sh.rowIdx[n] = r;
                    sh.mask[n] = sh.mask[r];
                    n++;
                }
            sh.R = n;
            for (int r = 0; r < n; r++) sh.done[r] = 0;
            sh.seen = 0;
            sh.off = 0;
            sh.W = 0;
        }
        __syncthreads();
        const int R = sh.R;
        int left = 0;  // lane c of wave 0: the unprocessed rows of column c
        if (tid < 64) {
            for (int r = 0; r < R; r++) left += (int)((sh.mask[r] >> tid) & 1ull);
            const u64 op = __ballot(left > 0), la = __ballot(left == 1);
            if (tid == 0) {
                sh.open = op;
                sh.last = la;
                sh.emptyCol = (op != (m == 64 ? ~0ull : (1ull << m) - 1ull)) ? 1 : 0;
            }
        }
        __syncthreads();
        // ---- plan ------------------------------------------------------------------------------------------------------------
        for (int i = 0; i < R; i++) {
            const u64 seen = sh.seen, open = sh.open, last = sh.last;
            unsigned key = 0xFFFFFFFFu;
            for (int r = tid; r < R; r += FS_THREADS) {
                if (sh.done[r]) continue;
                const u64 n = sh.mask[r], reach = (seen | n) & open;
                const unsigned kk = ((unsigned)__popcll(reach & ~(n & last)) << 18) | ((unsigned)__popcll(reach) << 11) | (unsigned)r;
                key = kk < key ? kk : key;
            }
            key = wave_min_u32(key);
            if (lane == 0) sh.key[wave] = key;
            __syncthreads();
            if (tid < 64) {
                unsigned best = sh.key[0];
                for (int w = 1; w < FS_THREADS / 64; w++) best = sh.key[w] < best ? sh.key[w] : best;
                const int r = (int)(best & 0x7FFu), Wsofar = sh.W;
                const u64 n = sh.mask[r];
                const u64 phi = seen & open, psi = phi | (n & ~seen), nxt = psi & ~(n & last);
                const int nPsi = __popcll(psi), nPhi = __popcll(phi);
                const u64 below = (1ull << tid) - 1ull;
                if (nPsi <= FS_W && Wsofar <= FS_W) {
                    FsStep &g = plan[i];
                    if ((psi >> tid) & 1ull) {
                        const int j = __popcll(psi & below);
                        g.col[j] = (signed char)tid;
                        g.posPhi[j] = (signed char)(((phi >> tid) & 1ull) ? __popcll(phi & below) : -1);
                        g.posNext[j] = (signed char)(((nxt >> tid) & 1ull) ? __popcll(nxt & below) : -1);
                    }
                    if (tid == 0) {
                        g.off = sh.off;
                        g.row = r;
                        g.nPsi = nPsi;
                        g.nPhi = nPhi;
                        g.nNext = __popcll(nxt);
                        g.pad = 0;
                    }
                }
                left -= (int)((n >> tid) & 1ull);
                const u64 op = __ballot(left > 0), la = __ballot(left == 1);
                if (tid == 0) {
                    if (nPsi <= FS_W && Wsofar <= FS_W) sh.off += 1ll << nPhi;
                    sh.W = nPsi > Wsofar ? nPsi : Wsofar;
                    sh.seen = seen | n;
                    sh.open = op;
                    sh.last = la;
                    sh.done[r] = 1;
                }
            }
            __syncthreads();
        }
        const int W = sh.W;
        if (tid == 0 && width) width[idx] = W;
        if (W > FS_W) {
            if (tid == 0 && info) info[idx] = -4;
            continue;
        }
        const long long offR = sh.off, total = offR + 1, need = total + (2ll << W);  // (the marginal tier's count: see above)
        if (need > wk.slotDoubles) {
            if (tid == 0 && info) info[idx] = -3;
            continue;
        }
        // ---- forward: the sums; where they end below the range, the count of the complete assignments over the same layers ----------
        fs_forward_sweep(sh, plan, x, nr, R, slot, offR, tid, false);
        const double Z = slot[offR];
        const bool ok = Z >= KB_RANGE_MIN_Z && !sh.emptyCol;
        if (!ok) {  // (uniform)
            __syncthreads();
            fs_forward_sweep(sh, plan, x, nr, R, slot, offR, tid, true);
            if (!sh.emptyCol && (slot[offR] > 0.0 || sh.lost)) {
                if (tid == 0 && info) info[idx] = KB_INFO_OUT_OF_RANGE;
                continue;
            }
        }
        if (!ok) {  // no draw: every thread answers the draws it owns
            for (int s = tid; s < nSample; s += FS_THREADS) {
                for (int c = 0; c < m; c++) asg[(long long)s * m + c] = -1;
                lt[s] = QNAN;
            }
            if (tid == 0) {
                if (logZ) logZ[idx] = -INF;
                if (info) info[idx] = 0;
            }
            continue;
        }
        // ---- the walk: rounds of FS_THREADS * FS_DPT draws, every round through the steps from the last to the first ---------------
        const u64 fk = src.frameKey(k);
        const u32 f0 = (u32)fk, f1 = (u32)(fk >> 32);
        const double lz = log(Z);
        for (int s0 = 0; s0 < nSample; s0 += FS_THREADS * FS_DPT) {  // (uniform)
            unsigned S[FS_DPT];  // the draw's state in Phi_{i+1}; F_R has the one state `empty`
#pragma unroll
            for (int d = 0; d < FS_DPT; d++) {
                S[d] = 0u;
                const int s = s0 + d * FS_THREADS + tid;
                if (s < nSample)
                    for (int c = 0; c < m; c++) asg[(long long)s * m + c] = -1;
            }
            for (int i = R - 1; i >= 0; i--) {
                fs_load_step(sh, plan, i, x, nr, tid, rowKey, false);
                __syncthreads();
                const unsigned psiM = (1u << sh.st.nPsi) - 1u, newM = sh.newM, closeM = sh.closeM, nrM = sh.nrM;
                const unsigned keepM = psiM & ~closeM, phiM = psiM & ~newM;
                const double *Fi = slot + sh.st.off;
                const double *Fn = slot + (i + 1 < R ? plan[i + 1].off : offR);
                const unsigned q = sh.q;
                const int subRow = sh.subRow;
#pragma unroll
                for (int d = 0; d < FS_DPT; d++) {
                    const int s = s0 + d * FS_THREADS + tid;
                    if (s >= nSample) continue;
                    const CsPhilox rnd = cs_philox4x32_10(sampleBase + (u32)s, 0x80000000u | (q >> 1), f0, f1, k0, k1);
                    const unsigned lo = (q & 1u) ? rnd.w[2] : rnd.w[0], hi = (q & 1u) ? rnd.w[3] : rnd.w[1];
                    const double u = (double)((((unsigned long long)hi << 32) | lo) >> 11) * 0x1.0p-53;
                    const unsigned T = fs_spread_bits(S[d], keepM) | closeM;
                    const unsigned nw = T & newM;
                    const unsigned base = fs_pack_bits(T, phiM);
                    const double tot = Fn[S[d]];
                    const double Tt = u * tot;
                    int take = -1;
                    if (nw == 0) {
                        double acc = Fi[base];
                        if (!(Tt < acc)) {
                            unsigned cols = T & nrM;
                            while (cols) {
                                const int j = __ffs(cols) - 1;
                                cols &= cols - 1u;
                                const double term = sh.aval[j] * Fi[base ^ (1u << sh.st.posPhi[j])];
                                acc = acc + term;
                                if (term > 0.0) take = j;
                                if (Tt < acc) break;
                            }
                        }
                        S[d] = take >= 0 ? base ^ (1u << sh.st.posPhi[take]) : base;
                    } else {  // a new column: the only way here is that the row takes it (two new columns: F_{i+1}[S] = 0, never entered)
                        if ((nw & (nw - 1u)) == 0) take = __ffs(nw) - 1;
                        S[d] = base;
                    }
                    if (take >= 0) asg[(long long)s * m + sh.st.col[take]] = subRow;
                }
                __syncthreads();  // (the step's staging is free again)
            }
            // the term of the draw: the columns in ascending order, every log from the cost itself
#pragma unroll
            for (int d = 0; d < FS_DPT; d++) {
                const int s = s0 + d * FS_THREADS + tid;
                if (s >= nSample) continue;
                double l = 0.0;
                for (int c = 0; c < m; c++) {
                    const int r = asg[(long long)s * m + c];  // (its own store; a walk from Z' > 0 leaves no column out)
                    l = l + ((unsigned)r < (unsigned)nr ? sh.colMin[c] - x[(long long)c * nr + r] : QNAN);
                }
                lt[s] = l - lz;
            }
        }
        if (tid == 0) {
            if (logZ) logZ[idx] = log(Z) - sh.sumCol;
            if (info) info[idx] = 1;
        }
    }
}

__global__ void __launch_bounds__(FS_THREADS)
frontier_sample_kernel(FrontierSamplePack p, const double *sub, const int *rowKeys, int nSample, u64 seed, u32 sampleBase,
                       int *assignLocal, double *logTerm, double *logZ, int *info, int *width, FrontierWork wk)
{
    __shared__ FsShared sh;
    frontier_sample_walk(sh, FsPackSource{p}, sub, rowKeys, nSample, seed, sampleBase, assignLocal, logTerm, logZ, info, width, wk);
}

// a workgroup without a cluster (blockIdx.x >= *count) returns at once
__global__ void __launch_bounds__(FS_THREADS)
frontier_sample_list_kernel(const HybridItem *list, const HybridKeyItem *keys, const int *count, const double *sub, const int *rowKeys,
                            int nSample, u64 seed, u32 sampleBase, int *assignLocal, double *logTerm, double *logZ, int *info,
                            int *width, FrontierWork wk)
{
    __shared__ FsShared sh;
    frontier_sample_walk(sh, FsListSource{list, keys, count}, sub, rowKeys, nSample, seed, sampleBase, assignLocal, logTerm, logZ, info,
                         width, wk);
}

}  // namespace

hipError_t launch_frontier_sample_pack(const FrontierSamplePack &p, const double *sub, const int *rowKeys, int nSample, u64 seed,
                                       u32 sampleBase, int *assignLocal, double *logTerm, double *logZ, int *info, int *width,
                                       const FrontierWork &w, int grid, hipStream_t stream)
{
    if (p.n <= 0) return hipSuccess;
    if (grid > p.n) grid = p.n;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(frontier_sample_kernel, dim3(grid), dim3(FS_THREADS), 0, stream, p, sub, rowKeys, nSample, seed, sampleBase,
                       assignLocal, logTerm, logZ, info, width, w);
    return hipGetLastError();
}

hipError_t launch_frontier_sample_list(const HybridItem *list, const HybridKeyItem *keys, const int *count, const double *sub,
                                       const int *rowKeys, int nSample, u64 seed, u32 sampleBase, int *assignLocal, double *logTerm,
                                       double *logZ, int *info, int *width, const FrontierWork &w, int grid, hipStream_t stream)
{
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL(frontier_sample_list_kernel, dim3(grid), dim3(FS_THREADS), 0, stream, list, keys, count, sub, rowKeys, nSample,
                       seed, sampleBase, assignLocal, logTerm, logZ, info, width, w);
    return hipGetLastError();
}

}  // namespace kb
