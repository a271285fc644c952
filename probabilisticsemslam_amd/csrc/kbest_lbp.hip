// kbest_lbp.hip -- beliefProb: the association probabilities of a frame by loopy belief propagation on the assignment model
// (the marginals of the Bethe approximation of the permanent), for frames of up to KBEST_LBP_MAX_COLS measurements and
// KBEST_MAX_DIM_WIDE rows.  gfx950, fp64, plain HIP C++.  DESIGN.md section 10.
//
// a = toProbs(cost) >= 0, R x C, exactly the matrix kbest_perm.hip works on (optional conditionCosts while loading, the exp and the
// expression of to_probs_kernel, all-zero rows left out).  nu = 1, then Jacobi sweeps:
//     x[r][c]   = a[r][c] nu[r][c]
//     s[r][c]   = sum_{r' != r} x[r'][c]
//     mu[r][c]  = a[r][c] / s[r][c]   where a[r][c] > 0 (s = 0: +inf, a forced entry), 0 elsewhere
//     nu'[r][c] = 1 / (1 + sum_{c' != c} mu[r][c'])
//     resid     = max over a[r][c] > 0 of |nu'[r][c] - nu[r][c]|
// until resid <= tol or maxIter sweeps (tol <= 0: exactly maxIter), then w = a nu, probs[c][min(r, nL)] += w[r][c] / sum_r w[r][c].
// Both exclusive sums are sums over the OTHER terms, never total minus own: every term is non-negative, nothing cancels and a
// forced entry gives no inf - inf.
//
// Work is sized to the frame: lane = row.  A launch has one wave per 64 rows of its bound (a frame-sized launch: ONE wave per
// frame, no barrier in a sweep), wave k holds rows 64 k .. 64 k + 63 of the frame ("chunk" k), every lane its own row of a, nu and
// of the two sweep buffers -- in LDS, or in the workgroup's slice of a work space in HBM (MODE 1): no lane ever reads another
// lane's entries, so the arithmetic and its order are the same in both.
//   * the sum over the other rows of a column: the wave's xor butterfly, where every lane keeps an inclusive and an exclusive
//     partial and adds the partner's inclusive one to both at every step; then the other chunks' totals in ascending order;
//   * the sum over the other columns of a row: lane-local, an ascending exclusive prefix plus a descending exclusive suffix;
//   * zero entries skip their terms: a bit mask of the non-zero columns per row (two 64-bit words per lane), and their union
//     over the chunk (in SGPRs) skips whole columns of a chunk -- the miss rows of a large frame are one chunk after another with
//     a column or two each.
// The order of every sum depends on the frame's own rows and columns only and there are no floating-point atomics: a frame's
// result does not depend on the batch it travels in, on the launch's bounds or on the storage mode, bit for bit.
//   * a column whose w sums to 0 (no finite entry; two columns forced onto one row): all probabilities 0 and iters = -2, not NaN.
#include <hip/hip_runtime.h>

#include <atomic>

#include "kbest_engine.h"
#include "kbest_wave.h"

namespace kb {

namespace {

constexpr double LB_GATE = 42.0;  // assignment.cpp:9
constexpr int LB_MAX_COLS = 128;  // KBEST_LBP_MAX_COLS: two mask words per lane

// x over the 64 lanes: incl = the sum of all lanes (the same bits in every lane: each step adds the two halves of a pair in
// either order), excl = the sum of the OTHER lanes.  All lanes must be active.  (xor 1, xor 2, then the other quad, the other
// half row -- after the steps before, every lane of it holds the same partial -- then xor 16 and xor 32.)
__device__ __forceinline__ void wave_xsum_f64(double x, double &incl, double &excl)
{
    double p;
    incl = x;
    p = dpp_f64<0xB1, 0xF>(incl);  excl = p;        incl = incl + p;  // quad_perm [1,0,3,2]
    p = dpp_f64<0x4E, 0xF>(incl);  excl = excl + p; incl = incl + p;  // quad_perm [2,3,0,1]
    p = dpp_f64<0x141, 0xF>(incl); excl = excl + p; incl = incl + p;  // row_half_mirror
    p = dpp_f64<0x140, 0xF>(incl); excl = excl + p; incl = incl + p;  // row_mirror
    p = __shfl_xor(incl, 16);      excl = excl + p; incl = incl + p;
    p = __shfl_xor(incl, 32);      excl = excl + p; incl = incl + p;
}

__device__ __forceinline__ double max_keep(double a, double b) { return b > a ? b : a; }

// fp64 max over the 64 lanes, wave-uniform.  All lanes must be active.
__device__ __forceinline__ double wave_max_f64(double x)
{
    x = max_keep(x, dpp_f64<0xB1, 0xF>(x));
    x = max_keep(x, dpp_f64<0x4E, 0xF>(x));
    x = max_keep(x, dpp_f64<0x141, 0xF>(x));
    x = max_keep(x, dpp_f64<0x140, 0xF>(x));
    x = max_keep(x, dpp_f64<0x142, 0xA>(x));
    x = max_keep(x, dpp_f64<0x143, 0xC>(x));
    return readlane_f64(x, 63);
}

struct LbpLds {  // byte offsets into the dynamic LDS
    int colMin, waveMin, ctl, resW, rawRow, flag, actRaw, tot, tot2, arr, total;
};

__host__ __device__ inline LbpLds lbp_lds(int mode, int maxRawRow, int maxCol)
{
    LbpLds l;
    const int W = (maxRawRow + 63) >> 6;
    int o = 0;
    l.colMin = o;  o += maxCol * 8;
    l.waveMin = o; o += 16 * 8;
    l.ctl = o;     o += 16;               // double blockMin; int nKept; int nAct
    l.resW = o;    o += 2 * 16 * 8;       // [sweep parity][wave]
    const int rows2 = (2 * maxRawRow + 7) & ~7;
    l.rawRow = o;  o += rows2;            // u16: raw row of every kept row
    l.flag = o;    o += rows2;            // u16: row kept / row active
    l.actRaw = o;  o += rows2;            // u16: raw row of every active (non-zero) row
    l.tot = o;     o += W * maxCol * 8;   // [chunk][column]: the chunks' column totals of a sweep, then of w
    l.tot2 = o;    o += W * maxCol * 8;   // [chunk][column]: the chunks' totals of the folded miss rows
    l.arr = o;     if (mode == 0) o += 4 * maxRawRow * maxCol * 8;  // a, nu, prefix, mu: [column][row]
    l.total = (o + 15) & ~15;
    return l;
}

__device__ __forceinline__ bool bit128(u64 lo, u64 hi, int c) { return (((c < 64) ? lo : hi) >> (c & 63)) & 1ull; }

// MODE 0: a, nu and the two sweep buffers in LDS; 1: in the HBM work space.
template <int MODE>
__global__ void __launch_bounds__(1024) kbest_lbp_kernel(LbpParams p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, NT = blockDim.x, lane = tid & 63, wave = tid >> 6, NWV = NT >> 6;
    const LbpLds L = lbp_lds(MODE, p.maxRawRow, p.maxCol);
    double *colMin = reinterpret_cast<double *>(smem + L.colMin);
    double *waveMin = reinterpret_cast<double *>(smem + L.waveMin);
    double *blockMin = reinterpret_cast<double *>(smem + L.ctl);
    int *nKeptW = reinterpret_cast<int *>(smem + L.ctl + 8);
    int *nActW = nKeptW + 1;
    double *resW = reinterpret_cast<double *>(smem + L.resW);
    unsigned short *rawRow = reinterpret_cast<unsigned short *>(smem + L.rawRow);
    unsigned short *flag = reinterpret_cast<unsigned short *>(smem + L.flag);
    unsigned short *actRaw = reinterpret_cast<unsigned short *>(smem + L.actRaw);
    double *tot = reinterpret_cast<double *>(smem + L.tot);
    double *tot2 = reinterpret_cast<double *>(smem + L.tot2);
    const int RS = p.maxRawRow, CS = p.maxCol;
    const long long plane = (long long)RS * CS;
    double *A = (MODE == 0) ? reinterpret_cast<double *>(smem + L.arr) : p.work + (long long)blockIdx.x * p.slotStride;
    double *V = A + plane, *T = V + plane, *U = T + plane;
    const double INF = d_inf();

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M;
        double *probOut = p.probs + p.probOff[b];
        const double *Cg = p.cost + p.costOff[b];
        // (uniform over the workgroup) a frame beyond what the launch was sized for: iters = -1 and untouched probs
        if (M < 1 || M > p.maxCol || M > LB_MAX_COLS || nLo < 0 || NR > p.maxRawRow) {
            if (tid == 0 && p.iters) p.iters[b] = -1;
            continue;
        }
        for (int i = tid; i < M * (nLo + 1); i += NT) probOut[i] = 0.0;  // (rows conditionCosts drops, zero rows: exactly 0.0)

        // ---- conditionCosts (assignment.cpp:439-525) while loading: as kbest_perm.hip has it --------------------------------------
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
                for (int c = 0; c < M; c++) good = good | (Cg[(long long)c * NR + r] <= colMin[c] + LB_GATE);
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
                if (lane == 0) *nKeptW = n;
            }
            __syncthreads();
            N = *nKeptW;
        } else {
            for (int r = tid; r < NR; r += NT) rawRow[r] = (unsigned short)r;
            N = NR;
            __syncthreads();
        }
        // ---- toProbs (:527-542) on the block handed over: its minimum first, then the rows that are non-zero after the gate -----
        {
            double m = INF;
            for (int i = tid; i < N * M; i += NT) {
                const int c = i / N, r = i - c * N;
                double x = Cg[(long long)c * NR + rawRow[r]];
                if (p.condition) x = (x <= colMin[c] + LB_GATE) ? (x - colMin[c]) : INF;  // (:490-494)
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
        }
        const double mn = *blockMin;
        for (int r = tid; r < N; r += NT) {
            const int raw = rawRow[r];
            bool any = false;
            for (int c = 0; c < M; c++) {
                double x = Cg[(long long)c * NR + raw];
                if (p.condition) x = (x <= colMin[c] + LB_GATE) ? (x - colMin[c]) : INF;
                any = any | (mn + LB_GATE > x);
            }
            flag[r] = any ? 1 : 0;
        }
        __syncthreads();
        if (wave == 0) {  // rows that are zero after the gate are left out
            int n = 0;
            for (int base = 0; base < N; base += 64) {
                const int r = base + lane;
                const bool on = r < N && flag[r] != 0;
                const u64 m2 = __ballot(on);
                if (on) actRaw[n + __popcll(m2 & ((1ull << lane) - 1ull))] = rawRow[r];
                n += __popcll(m2);
            }
            if (lane == 0) *nActW = n;
        }
        __syncthreads();
        const int Ra = *nActW;
        const int nCh = (Ra + 63) >> 6;  // chunks of 64 rows: wave k holds chunk k (the launch has a wave per 64 rows of its bound)
        const bool multi = nCh > 1;      // (the frame's own property: so is every order of summation below)
        const int row = wave * 64 + lane;
        const bool on = row < Ra;
        const int raw = on ? actRaw[row] : 0;

        // ---- every lane loads its own row: a = exp(min - c) where min + 42 > c (:536-540, as to_probs_kernel has it), nu = 1 -------
        u64 lm0 = 0, lm1 = 0, cm0 = 0, cm1 = 0;  // non-zero columns of the lane's row, and of the whole chunk
        for (int c = 0; c < M; c++) {
            bool nz = false;
            if (on) {
                double x = Cg[(long long)c * NR + raw];
                if (p.condition) x = (x <= colMin[c] + LB_GATE) ? (x - colMin[c]) : INF;
                const double av = (mn + LB_GATE > x) ? exp(mn - x) : 0.0;
                A[(long long)c * RS + row] = av;
                V[(long long)c * RS + row] = 1.0;
                nz = av > 0.0;
            }
            const u64 bitc = 1ull << (c & 63);
            const bool anyc = __ballot(nz) != 0ull;
            if (c < 64) { lm0 |= nz ? bitc : 0ull; cm0 |= anyc ? bitc : 0ull; }
            else        { lm1 |= nz ? bitc : 0ull; cm1 |= anyc ? bitc : 0ull; }
            if (lane == 0) {
                tot[wave * CS + c] = 0.0;
                tot2[wave * CS + c] = 0.0;
            }
        }
        cm0 = uni64(cm0);
        cm1 = uni64(cm1);

        // ---- the sweeps -----------------------------------------------------------------------------------------------------------
        int it = 0;
        double resid = 0.0;
        while (it < p.maxIter) {
            if (multi) {  // this chunk's share of every column: the exclusive part stays with the lane, the total goes to the others
                for (int c = 0; c < M; c++) {
                    if (!bit128(cm0, cm1, c)) continue;  // (uniform over the wave; the total stays 0)
                    const bool has = bit128(lm0, lm1, c);
                    const long long ix = (long long)c * RS + row;
                    const double x = has ? A[ix] * V[ix] : 0.0;
                    double incl, excl;
                    wave_xsum_f64(x, incl, excl);
                    if (has) T[ix] = excl;
                    if (lane == 0) tot[wave * CS + c] = incl;
                }
                __syncthreads();
            }
            double pre = 0.0;  // sum of mu over the columns before c
            for (int c = 0; c < M; c++) {
                if (!bit128(cm0, cm1, c)) continue;
                const bool has = bit128(lm0, lm1, c);
                const long long ix = (long long)c * RS + row;
                const double av = has ? A[ix] : 0.0;
                double s;
                if (!multi) {
                    const double x = has ? av * V[ix] : 0.0;
                    double incl;
                    wave_xsum_f64(x, incl, s);
                } else {
                    s = has ? T[ix] : 0.0;
                    for (int j = 0; j < nCh; j++)
                        if (j != wave) s = s + tot[j * CS + c];
                }
                if (has) {
                    const double mu = av / s;  // (s = 0: +inf)
                    T[ix] = pre;
                    U[ix] = mu;
                    pre = pre + mu;
                }
            }
            double suf = 0.0, res = 0.0;  // sum of mu over the columns after c
            for (int c = M - 1; c >= 0; c--) {
                if (!bit128(cm0, cm1, c)) continue;
                if (bit128(lm0, lm1, c)) {
                    const long long ix = (long long)c * RS + row;
                    const double nu = 1.0 / (1.0 + (T[ix] + suf));
                    res = max_keep(res, fabs(nu - V[ix]));
                    V[ix] = nu;
                    suf = suf + U[ix];
                }
            }
            res = wave_max_f64(res);
            if (NWV > 1) {  // (two buffers: a wave may write the next sweep's while another still reads this one's)
                double *rw = resW + (it & 1) * 16;
                if (lane == 0) rw[wave] = res;
                __syncthreads();
                res = rw[0];
                for (int w = 1; w < NWV; w++) res = max_keep(res, rw[w]);
            }
            resid = res;
            it++;
            if (p.tol > 0.0 && resid <= p.tol) break;
        }

        // ---- w = a nu, its column sums, the probabilities -------------------------------------------------------------------------
        for (int c = 0; c < M; c++) {
            if (!bit128(cm0, cm1, c)) continue;
            const bool has = bit128(lm0, lm1, c);
            const long long ix = (long long)c * RS + row;
            const double w = has ? A[ix] * V[ix] : 0.0;
            double incl, excl;
            wave_xsum_f64(w, incl, excl);
            if (lane == 0) tot[wave * CS + c] = incl;
        }
        __syncthreads();
        bool feasible = Ra > 0;
        for (int c = 0; c < M; c++) {  // (every thread the same sums: uniform)
            double S = 0.0;
            if (nCh > 0) S = tot[c];
            for (int j = 1; j < nCh; j++) S = S + tot[j * CS + c];
            feasible = feasible & (S > 0.0);
        }
        for (int c = 0; c < M; c++) {
            if (!bit128(cm0, cm1, c)) continue;
            const bool has = feasible && bit128(lm0, lm1, c);
            const long long ix = (long long)c * RS + row;
            double q = 0.0;
            if (has) {
                double S = tot[c];
                for (int j = 1; j < nCh; j++) S = S + tot[j * CS + c];
                q = (A[ix] * V[ix]) / S;
                if (raw < nLo) probOut[c * (nLo + 1) + raw] = q;  // scatter back to the caller's landmark numbering (:68-74)
            }
            double incl, excl;
            wave_xsum_f64((has && raw >= nLo) ? q : 0.0, incl, excl);  // rows r >= nL fold into slot nL
            if (lane == 0) tot2[wave * CS + c] = incl;
        }
        __syncthreads();
        if (feasible)
            for (int c = tid; c < M; c += NT) {
                double m = tot2[c];
                for (int j = 1; j < nCh; j++) m = m + tot2[j * CS + c];
                probOut[c * (nLo + 1) + nLo] = m;
            }
        if (tid == 0) {
            if (p.iters) p.iters[b] = feasible ? it : -2;
            if (p.resid) p.resid[b] = resid;
        }
        __syncthreads();
    }
}

template <int MODE>
hipError_t launch_mode(const LbpParams &p, int grid, int threads, int lds, hipStream_t stream)
{
    static std::atomic<int> granted[16];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (lds > granted[dev & 15].load(std::memory_order_relaxed)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kbest_lbp_kernel<MODE>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        granted[dev & 15].store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((kbest_lbp_kernel<MODE>), dim3(grid), dim3(threads), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

LbpPlan lbp_plan(int maxRawRow, int maxCol, int ldsLimit)
{
    LbpPlan pl;
    pl.threads = 64 * ((maxRawRow + 63) >> 6);
    const long long lds0 = (long long)lbp_lds(1, maxRawRow, maxCol).total + 4ll * maxRawRow * maxCol * 8;
    if (lds0 <= ldsLimit) { pl.mode = 0; pl.lds = lbp_lds(0, maxRawRow, maxCol).total; pl.slotDoubles = 0; }
    else { pl.mode = 1; pl.lds = lbp_lds(1, maxRawRow, maxCol).total; pl.slotDoubles = 4ll * maxRawRow * maxCol; }
    return pl;
}

hipError_t launch_kbest_lbp(const LbpParams &p, const LbpPlan &pl, int grid, hipStream_t stream)
{
    return pl.mode == 0 ? launch_mode<0>(p, grid, pl.threads, pl.lds, stream) : launch_mode<1>(p, grid, pl.threads, pl.lds, stream);
}

}  // namespace kb
