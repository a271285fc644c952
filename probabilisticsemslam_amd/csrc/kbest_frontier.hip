// kbest_frontier.hip -- the fourth tier of the exact subset sums: a cluster of up to KBEST_FRONTIER_MAX_COLS = 64 measurements
// whose rows, taken in a good order, never keep more than KBEST_FRONTIER_MAX_WIDTH = 16 columns open.  One workgroup per cluster,
// ONE launch for the clusters of a call.  gfx950, fp64, plain HIP C++.  DESIGN.md section 14.
//
// Input and scaling are those of kbest_bigcluster.hip: the (nL_k + m_k) x m_k column-major sub-block of
// kbest_clustered_partial_batch_f64_dev, +inf for a zero, rows that are all +inf left out, a'[r][c] = exp(colMin_c - x[r][c]),
// log Z = log Z' - sum_c colMin_c.  a' is not stored: a step needs the at most 16 entries of its row and computes them again.
// The tier answers while Z' >= KB_RANGE_MIN_Z = 2^-970 (every term within 2^-52 of Z' is then a normal double).  Below that, Z' = 0
// included, the forward sweep runs once more with every non-zero entry 1: it counts the complete assignments of the pattern, and a
// sum of ones cannot underflow.  None (and no finite entry whose a' is 0): info 0.  Else the cluster is declined, info -5.
//
// A column is a state bit only between its first and its last non-zero row: before, it is unused; after, it must be used.
//   plan      N_r = the non-zero columns of row r (one 64-bit word), left[c] = unprocessed rows with c in N_r, seen = the union of
//             N_r over the processed rows.  Step i takes the unprocessed row with the smallest (f, pk, r),
//                 pk(r) = |(seen | N_r) & {left > 0}|,   f(r) = |(seen | N_r) & {left - [c in N_r] > 0}|
//             (lane = candidate row, workgroup arg-min of the packed key).  Phi_i = seen & {left > 0} are the open columns before
//             the step, Psi_i = Phi_i | (N_r \ seen) the ones during it, closing_i the columns of N_r with left = 1; state bit j
//             is the j-th column of the set in ascending order.  W = max |Psi_i|.  A step of the plan: its row, the column of
//             every bit of Psi_i and that bit's place in Phi_i and in Phi_{i+1}, or -1.
//   forward   F_0 = {empty: 1}; one thread per S of Phi_{i+1}, T = S | closing_i in Psi_i:
//                 F_{i+1}[S] = [T & new = 0] F_i[T] + sum_{c in T & N_r, (T \ c) & new = 0, c ascending} a'[r][c] F_i[T \ c]
//             every layer stays (2^|Phi_i| doubles each); Z' = F_R[empty].
//   backward  G_R = {empty: 1}; one thread per S of Phi_i, strided: with g(S, c) = [closing_i in S | c] G_{i+1}[(S | c) in Phi_{i+1}]
//                 G_i[S] = g(S, none) + sum_{c in N_r \ S} a'[r][c] g(S, c),     w[r][c] = a'[r][c] sum_S F_i[S] g(S, c)
//             in two buffers.  The sum for w has the fixed shape of the other tiers: a thread takes S = t, t + 256, ..., the wave
//             butterfly, the four waves in ascending order.  probs[c][min(r, nL_k)] += w / Z'; the rows >= nL_k add up in the
//             order of the sweep.
// No workgroup waits for another (no grid barrier, no flag, no cooperative launch) and there are no floating-point atomics: the
// order of every sum depends on the cluster alone, so a cluster gives the same bits alone, anywhere in a batch and under any cap.
// info: 1 answered; 0: no complete assignment (zeros, log Z = -inf); -5: Z' < 2^-970 although there is one; -4: W > 16; -3: the
// layers sum_i 2^|Phi_i| + 2 2^W doubles exceed the slot -- all from the cluster alone, and a refused cluster's outputs are not touched.
// Two entry points, one sweep (frontier_sweep<Source>): frontier_kernel takes its clusters from a kernel-argument pack,
// frontier_list_kernel from the list kbest_hybrid.hip gathers on the device.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_wave_sum.h"

namespace kb {

namespace {

constexpr int FR_THREADS = KB_FRONTIER_THREADS;
constexpr int FR_W = KB_FRONTIER_MAX_WIDTH;
constexpr int FR_ROWS = KB_FRONTIER_MAX_ROWS;

struct FrontierStep {  // KB_FRONTIER_STEP_DOUBLES * 8 bytes
    long long off;     // F_i, in doubles from the slot
    int row;           // the counting row it takes
    int nPsi, nPhi, nNext;
    int pad;
    signed char col[FR_W], posPhi[FR_W], posNext[FR_W];  // per bit of Psi_i
};
static_assert(sizeof(FrontierStep) == KB_FRONTIER_STEP_DOUBLES * 8, "FrontierStep");

// the bits of v at the places of mask, packed / the low bits of v spread to the places of mask (mask uniform, at most 16 bits)
__device__ __forceinline__ unsigned pack_bits(unsigned v, unsigned mask)
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
__device__ __forceinline__ unsigned spread_bits(unsigned v, unsigned mask)
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

struct FrShared {
    u64 mask[FR_ROWS];          // N_r of the counting rows
    int rowIdx[FR_ROWS];        // their rows in the sub-block
    unsigned char done[FR_ROWS];
    double colMin[KB_FRONTIER_MAX_COLS], miss[KB_FRONTIER_MAX_COLS];
    double red[(FR_THREADS / 64) * FR_W];
    double aval[FR_W];          // a'[r][column of bit j], 0 outside N_r
    u64 seen, open, last;
    long long off, total;
    double sumCol;
    unsigned key[FR_THREADS / 64];
    unsigned nrM, newM, closeM;  // bits of Psi_i: in N_r / not in Phi_i / not in Phi_{i+1}
    int R, W, emptyCol;
    int lost;                    // a finite entry whose a' is 0
    FrontierStep st;
};

// the step's description from the plan, its a' (unit: 1 for every non-zero one) and its masks: wave 0; a barrier follows
__device__ __forceinline__ void load_step(FrShared &sh, const FrontierStep *plan, int i, const double *x, int nr, int tid, bool unit)
{
    if (tid < 64) {
        const FrontierStep &g = plan[i];
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
        }
    }
}

// F_0 .. F_R of a planned cluster into its slot; unit: every non-zero a' is 1, and F_R[empty] counts the complete assignments
__device__ __forceinline__ void forward_sweep(FrShared &sh, const FrontierStep *plan, const double *x, int nr, int R, double *slot,
                                              long long offR, int tid, bool unit)
{
    if (tid == 0) slot[0] = 1.0;
    __syncthreads();
    for (int i = 0; i < R; i++) {
        load_step(sh, plan, i, x, nr, tid, unit);
        __syncthreads();
        const unsigned psiM = (1u << sh.st.nPsi) - 1u, newM = sh.newM, closeM = sh.closeM, nrM = sh.nrM;
        const unsigned keepM = psiM & ~closeM, phiM = psiM & ~newM;
        const double *Fi = slot + sh.st.off;
        double *Fn = slot + (i + 1 < R ? plan[i + 1].off : offR);
        const int nS = 1 << sh.st.nNext;
        for (int S = tid; S < nS; S += FR_THREADS) {
            const unsigned T = spread_bits((unsigned)S, keepM) | closeM;
            const unsigned nw = T & newM;
            const unsigned base = pack_bits(T, phiM);
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

// Where the clusters of a launch come from: the kernel-argument pack of kbest_frontier_probs_f64_dev, or the list
// hybrid_gather_kernel (kbest_hybrid.hip) left in HBM with its count word.  The sweep below is the same code for both.
struct PackSource {
    const FrontierPack &p;
    __device__ __forceinline__ int n() const { return p.n; }
    __device__ __forceinline__ bool sent(int) const { return true; }
    __device__ __forceinline__ int m(int k) const { return p.c[k].m; }
    __device__ __forceinline__ int nL(int k) const { return p.c[k].nL; }
    __device__ __forceinline__ long long subOff(int k) const { return p.c[k].subOff; }
    __device__ __forceinline__ long long probOff(int k) const { return p.c[k].probOff; }
    __device__ __forceinline__ int idx(int k) const { return p.base + k; }
};
struct ListSource {
    const HybridItem *list;
    const int *count;
    __device__ __forceinline__ int n() const { return *count; }
    __device__ __forceinline__ bool sent(int k) const { return list[k].sent != 0; }
    __device__ __forceinline__ int m(int k) const { return list[k].m; }
    __device__ __forceinline__ int nL(int k) const { return list[k].nL; }
    __device__ __forceinline__ long long subOff(int k) const { return list[k].subOff; }
    __device__ __forceinline__ long long probOff(int k) const { return list[k].probOff; }
    __device__ __forceinline__ int idx(int k) const { return k; }
};

template <class Source>
__device__ __forceinline__ void frontier_sweep(FrShared &sh, const Source &src, const double *sub, double *probs, double *logZ,
                                               int *info, int *width, const FrontierWork &wk)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *slot = wk.layers + (long long)blockIdx.x * wk.slotDoubles;
    FrontierStep *plan = reinterpret_cast<FrontierStep *>(wk.plan + (long long)blockIdx.x * wk.planDoubles);
    const double INF = d_inf();
    const int n = src.n();
    for (int k = blockIdx.x; k < n; k += gridDim.x) {
        if (!src.sent(k)) continue;  // (uniform)
        const int m = src.m(k), nL = src.nL(k), nr = nL + m, idx = src.idx(k);
        const double *x = sub + src.subOff(k);
        double *out = probs + src.probOff(k);
        __syncthreads();  // (the previous cluster is done with the shared arrays)
        if ((long long)nr * KB_FRONTIER_STEP_DOUBLES > wk.planDoubles || nr > FR_ROWS || m > KB_FRONTIER_MAX_COLS) {
            if (tid == 0 && info) info[idx] = -3;  // (the host entry never lets this happen)
            continue;
        }
        // ---- setup: column minima, the rows that count, the row masks ------------------------------------------------------
        if (tid < m) {
            double mn = INF;
            for (int r = 0; r < nr; r++) mn = min_keep(mn, x[(long long)tid * nr + r]);
            sh.colMin[tid] = mn;
        }
        if (tid < KB_FRONTIER_MAX_COLS) sh.miss[tid] = 0.0;
        if (tid == 0) sh.lost = 0;
        __syncthreads();
        for (int r = tid; r < nr; r += FR_THREADS) {
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
            for (int r = tid; r < R; r += FR_THREADS) {
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
                for (int w = 1; w < FR_THREADS / 64; w++) best = sh.key[w] < best ? sh.key[w] : best;
                const int r = (int)(best & 0x7FFu), Wsofar = sh.W;
                const u64 n = sh.mask[r];
                const u64 phi = seen & open, psi = phi | (n & ~seen), nxt = psi & ~(n & last);
                const int nPsi = __popcll(psi), nPhi = __popcll(phi);
                const u64 below = (1ull << tid) - 1ull;
                if (nPsi <= FR_W && Wsofar <= FR_W) {
                    FrontierStep &g = plan[i];
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
                    if (nPsi <= FR_W && Wsofar <= FR_W) sh.off += 1ll << nPhi;
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
        if (W > FR_W) {
            if (tid == 0 && info) info[idx] = -4;
            continue;
        }
        const long long offR = sh.off, total = offR + 1, need = total + (2ll << W);  // F_R is one double
        if (need > wk.slotDoubles) {
            if (tid == 0 && info) info[idx] = -3;
            continue;
        }
        // ---- forward: the sums; where they end below the range, the count of the complete assignments over the same layers ----------
        forward_sweep(sh, plan, x, nr, R, slot, offR, tid, false);
        const double Z = slot[offR];
        const bool ok = Z >= KB_RANGE_MIN_Z && !sh.emptyCol;
        bool declined = false;
        if (!ok) {  // (uniform)
            __syncthreads();
            forward_sweep(sh, plan, x, nr, R, slot, offR, tid, true);
            declined = !sh.emptyCol && (slot[offR] > 0.0 || sh.lost);
        }
        if (declined) {
            if (tid == 0 && info) info[idx] = KB_INFO_OUT_OF_RANGE;
            continue;
        }
        for (int i = tid; i < m * (nL + 1); i += FR_THREADS) out[i] = 0.0;
        if (!ok) {
            if (tid == 0) {
                if (logZ) logZ[idx] = -INF;
                if (info) info[idx] = 0;
            }
            continue;
        }
        // ---- backward with the marginals -------------------------------------------------------------------------------------
        double *Gbuf = slot + total;
        if (tid == 0) Gbuf[0] = 1.0;
        for (int i = R - 1, t = 0; i >= 0; i--, t++) {
            load_step(sh, plan, i, x, nr, tid, false);
            __syncthreads();
            const unsigned psiM = (1u << sh.st.nPsi) - 1u, newM = sh.newM, closeM = sh.closeM, nrM = sh.nrM;
            const unsigned keepM = psiM & ~closeM, phiM = psiM & ~newM;
            const double *Fi = slot + sh.st.off;
            const double *Gc = Gbuf + ((long long)(t & 1) << W);       // G_{i+1}
            double *Gn = Gbuf + ((long long)((t & 1) ^ 1) << W);       // G_i
            const int nS = 1 << sh.st.nPhi;
            double acc[FR_W];
#pragma unroll
            for (int j = 0; j < FR_W; j++) acc[j] = 0.0;
            for (int S = tid; S < nS; S += FR_THREADS) {
                const unsigned Tb = spread_bits((unsigned)S, phiM);
                const double f = Fi[S];
                const unsigned cand = nrM & ~Tb, lacks = closeM & ~Tb;
                const unsigned gb = pack_bits(Tb, keepM);
                double g = lacks == 0 ? Gc[gb] : 0.0;
#pragma unroll
                for (int j = 0; j < FR_W; j++)
                    if (((cand >> j) & 1u) && (lacks & ~(1u << j)) == 0) {  // (the places are ranks: one bit more, one place more)
                        const int pn = sh.st.posNext[j];
                        const double gv = Gc[pn < 0 ? gb : gb | (1u << pn)];
                        acc[j] = acc[j] + f * gv;
                        g = g + sh.aval[j] * gv;
                    }
                Gn[S] = g;
            }
#pragma unroll
            for (int j = 0; j < FR_W; j++)
                if ((nrM >> j) & 1u) {  // (uniform)
                    const double s = wave_sum63_f64(acc[j]);
                    if (lane == 63) sh.red[wave * FR_W + j] = s;
                }
            __syncthreads();
            if (tid < FR_W && ((nrM >> tid) & 1u)) {
                double s = sh.red[tid];
                for (int w = 1; w < FR_THREADS / 64; w++) s = s + sh.red[w * FR_W + tid];
                const double wv = sh.aval[tid] * s;
                const int c = sh.st.col[tid], r = sh.rowIdx[sh.st.row];
                if (r < nL) out[(long long)c * (nL + 1) + r] = wv / Z;
                else sh.miss[c] = sh.miss[c] + wv;
            }
            __syncthreads();
        }
        if (tid < m) out[(long long)tid * (nL + 1) + nL] = sh.miss[tid] / Z;
        if (tid == 0) {
            if (logZ) logZ[idx] = log(Z) - sh.sumCol;
            if (info) info[idx] = 1;
        }
    }
}

__global__ void __launch_bounds__(FR_THREADS)
frontier_kernel(FrontierPack p, const double *sub, double *probs, double *logZ, int *info, int *width, FrontierWork wk)
{
    __shared__ FrShared sh;
    frontier_sweep(sh, PackSource{p}, sub, probs, logZ, info, width, wk);
}

// a workgroup without a cluster (blockIdx.x >= *count) returns at once
__global__ void __launch_bounds__(FR_THREADS)
frontier_list_kernel(const HybridItem *list, const int *count, const double *sub, double *probs, double *logZ, int *info, int *width,
                     FrontierWork wk)
{
    __shared__ FrShared sh;
    frontier_sweep(sh, ListSource{list, count}, sub, probs, logZ, info, width, wk);
}

}  // namespace

hipError_t launch_frontier_pack(const FrontierPack &p, const double *sub, double *probs, double *logZ, int *info, int *width,
                                const FrontierWork &w, int grid, hipStream_t stream)
{
    if (p.n <= 0) return hipSuccess;
    if (grid > p.n) grid = p.n;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(frontier_kernel, dim3(grid), dim3(FR_THREADS), 0, stream, p, sub, probs, logZ, info, width, w);
    return hipGetLastError();
}

hipError_t launch_frontier_list(const HybridItem *list, const int *count, const double *sub, double *probs, double *logZ, int *info,
                                int *width, const FrontierWork &w, int grid, hipStream_t stream)
{
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL(frontier_list_kernel, dim3(grid), dim3(FR_THREADS), 0, stream, list, count, sub, probs, logZ, info, width, w);
    return hipGetLastError();
}

}  // namespace kb
