// kbest_bigcluster.hip -- the third tier of the exact subset sums: ONE cluster over the whole chip, its layers in HBM, for the
// clusters of up to KBEST_BIGCLUSTER_MAX_SIZE = 20 measurements the partial mode of kbest_cluster.hip hands out.
// gfx950, fp64, plain HIP C++.  DESIGN.md section 13.
//
// Per cluster the input is the (nL_k + m_k) x m_k column-major sub-block of kbest_clustered_partial_batch_f64_dev: the value
// toProbs is applied to, +inf for a zero.  The matrix is a'[r][c] = exp(colMin_c - x[r][c]), colMin_c the column's smallest
// finite entry inside the sub-block; rows that are all +inf are left out.  A column factor is the only rescaling that commutes
// with the recurrence (rows may stay unassigned, so a row factor is not uniform; F[empty set] = 1 in every layer, so a layer factor
// is none), it leaves the marginals alone and log Z = log Z' - sum_c colMin_c in the units a = exp(-x).  Every entry lies in
// (0, 1] and every column holds a 1: Z' leaves the normal doubles only when every complete assignment of the cluster costs about
// 700 more than the sum of its column minima.  The tier answers while Z' >= KB_RANGE_MIN_Z = 2^-970 (every term within 2^-52 of
// Z' is then a normal double).  Below that, Z' = 0 included, bc_verdict counts the complete assignments of the pattern a' > 0 by
// the same recurrence with every non-zero entry 1 -- a sum of ones cannot underflow: none, and no finite entry whose a' is 0, is
// info 0 (zeros, log Z = -inf); else the cluster is declined, info KB_INFO_OUT_OF_RANGE = -5, its outputs untouched.
//
// Launches of one stream order the layers; no kernel waits for another workgroup (no grid barrier, no flag, no cooperative launch):
//   bc_setup      one workgroup per cluster: column minima, the rows that count, a', the row masks
//   bc_init       F_0 = G_R = the indicator of the empty set
//   bc_forward    one launch per row i, one thread per column subset S:
//                     F_{i+1}[S] = F_i[S] + sum_{c in S, a'[i][c] > 0, c ascending} a'[i][c] F_i[S \ c];  all layers F_0 .. F_R stay
//   bc_backward   one launch per row i = R-1 .. 0: w[i][c] = a'[i][c] sum_{S without c} F_i[S] G_{i+1}[all \ S \ c] for every
//                 non-zero column, and G_i from G_{i+1} in the other of two buffers.  The sum has a fixed shape: a thread takes
//                 BC_SPT subsets BC_THREADS apart, the wave butterfly, the four waves in ascending order, then one partial per
//                 workgroup in HBM
//   bc_verdict    one workgroup per cluster: answered (the outputs zeroed), infeasible or out of range (above); the count takes
//                 the two buffers of G, which the backward sweep is done with
//   bc_rows       sums the partials of a row in ascending workgroup order and writes the landmark rows back
//   bc_finish     the rows >= nL_k into slot nL_k, log Z, info
// Workgroups per cluster follow from m_k alone -- never from the device -- and there are no floating-point atomics: the order of
// every sum depends on (m_k, R_k) only; a cluster gives the same bits alone, in any batch and under any cap.  Several clusters
// share the launches (grid.y = cluster) as far as the work space holds their layers.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_wave_sum.h"

namespace kb {

namespace {

constexpr int BC_MAX = 20;        // KBEST_BIGCLUSTER_MAX_SIZE
constexpr int BC_THREADS = 256;   // every kernel but bc_rows / bc_finish
constexpr int BC_SPT = 4;         // subsets per thread of the backward sweep: BC_THREADS * BC_SPT subsets per workgroup

struct BcView {  // one cluster's part of the work space
    double *a, *colMin, *sumCol, *miss, *part, *F, *G;
    int *R, *rowIdx, *mask;
    int m, nL, rows, nsub, nwg;
};

__device__ __forceinline__ BcView bc_view(const BigClusterPack &p, int k, double *layers, double *small)
{
    const BigClusterDesc &d = p.c[k];
    const BigClusterSmall s = bigcluster_small(d.m, d.rows);
    BcView v;
    double *base = small + d.smallOff;
    v.a = base + s.a;
    v.colMin = base + s.colMin;
    v.sumCol = base + s.sumCol;
    v.miss = base + s.miss;
    v.part = base + s.part;
    v.R = reinterpret_cast<int *>(base + s.ints);
    v.rowIdx = v.R + 1;
    v.mask = v.rowIdx + d.rows;
    v.m = d.m;
    v.nL = d.nL;
    v.rows = d.rows;
    v.nsub = 1 << d.m;
    v.nwg = bigcluster_workgroups(d.m);
    v.F = layers + d.layerOff;
    v.G = v.F + (long long)(d.rows + 1) * v.nsub;
    return v;
}

__global__ void __launch_bounds__(BC_THREADS)
bc_setup_kernel(BigClusterPack p, const double *sub, double *layers, double *small)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    const BcView v = bc_view(p, k, layers, small);
    const double *x = sub + p.c[k].subOff;
    const int m = v.m, nr = v.rows;
    const double INF = d_inf();
    for (int i = tid; i < m * m; i += BC_THREADS) v.miss[i] = 0.0;
    for (int c = tid; c < m; c += BC_THREADS) {  // the column's smallest finite entry
        double mn = INF;
        for (int r = 0; r < nr; r++) mn = min_keep(mn, x[(long long)c * nr + r]);
        v.colMin[c] = mn;
    }
    for (int r = tid; r < nr; r += BC_THREADS) {  // rows that are all +inf are left out
        bool any = false;
        for (int c = 0; c < m; c++) any = any | (x[(long long)c * nr + r] < INF);
        v.mask[r] = any ? 1 : 0;  // (until the masks are written below)
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int c = 0; c < m; c++) s = s + (v.colMin[c] < INF ? v.colMin[c] : 0.0);
        *v.sumCol = s;
        int n = 0;
        for (int r = 0; r < nr; r++)
            if (v.mask[r]) v.rowIdx[n++] = r;
        *v.R = n;
    }
    __syncthreads();
    const int R = *v.R;
    for (int i = tid; i < R * m; i += BC_THREADS) {
        const int r = i / m, c = i - r * m;
        const double e = x[(long long)c * nr + v.rowIdx[r]];
        v.a[i] = (e < INF) ? exp(v.colMin[c] - e) : 0.0;
    }
    __syncthreads();
    for (int r = tid; r < R; r += BC_THREADS) {
        unsigned mk = 0;
        for (int c = 0; c < m; c++) mk |= (v.a[r * m + c] > 0.0) ? (1u << c) : 0u;
        v.mask[r] = (int)mk;
    }
}

__global__ void __launch_bounds__(BC_THREADS)
bc_init_kernel(BigClusterPack p, double *layers, double *small)
{
    const BcView v = bc_view(p, blockIdx.y, layers, small);
    const int S = blockIdx.x * BC_THREADS + threadIdx.x;
    if (S >= v.nsub) return;
    const double e = (S == 0) ? 1.0 : 0.0;
    v.F[S] = e;
    v.G[S] = e;
}

__global__ void __launch_bounds__(BC_THREADS)
bc_forward_kernel(BigClusterPack p, int i, double *layers, double *small)
{
    const BcView v = bc_view(p, blockIdx.y, layers, small);
    const int S = blockIdx.x * BC_THREADS + threadIdx.x;
    if (i >= *v.R || S >= v.nsub) return;
    const double *ar = v.a + i * v.m;
    const double *Fi = v.F + (long long)i * v.nsub;
    double val = 0.0;
    if (__popc(S) <= i + 1) {  // (more columns than rows so far: 0)
        val = Fi[S];
        unsigned cols = (unsigned)S & (unsigned)v.mask[i];
        while (cols) {
            const int c = __ffs(cols) - 1;
            cols &= cols - 1u;
            val = val + ar[c] * Fi[S ^ (1 << c)];
        }
    }
    v.F[(long long)(i + 1) * v.nsub + S] = val;
}

// step t = 0, 1, ...: the row R - 1 - t of every cluster that has one
__global__ void __launch_bounds__(BC_THREADS)
bc_backward_kernel(BigClusterPack p, int t, double *layers, double *small)
{
    __shared__ double red[(BC_THREADS / 64) * BC_MAX];
    const BcView v = bc_view(p, blockIdx.y, layers, small);
    const int R = *v.R, r = R - 1 - t, wg = blockIdx.x;
    if (r < 0 || wg >= v.nwg) return;  // (uniform over the workgroup)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = v.m, nsub = v.nsub;
    const unsigned full = (unsigned)nsub - 1u, mk = (unsigned)v.mask[r];
    const double *ar = v.a + r * m;
    const double *Fr = v.F + (long long)r * nsub;
    const double *Gc = v.G + (long long)(t & 1) * nsub;  // G_{r+1}
    double *Gn = v.G + (long long)((t & 1) ^ 1) * nsub;  // G_r
    double acc[BC_MAX];
#pragma unroll
    for (int c = 0; c < BC_MAX; c++) acc[c] = 0.0;
    const int S0 = wg * (BC_THREADS * BC_SPT) + tid;
    double fv[BC_SPT];
#pragma unroll
    for (int j = 0; j < BC_SPT; j++) fv[j] = (S0 + j * BC_THREADS < nsub) ? Fr[S0 + j * BC_THREADS] : 0.0;
#pragma unroll
    for (int j = 0; j < BC_SPT; j++) {
        const double f = fv[j];
        if (f == 0.0) continue;
        const unsigned S = (unsigned)(S0 + j * BC_THREADS);
        const unsigned cols = mk & ~S;
        const unsigned comp = full ^ S;
#pragma unroll
        for (int c = 0; c < BC_MAX; c++)
            if ((cols >> c) & 1u) acc[c] = acc[c] + f * Gc[comp ^ (1u << c)];
    }
    if (r > 0) {
        const int left = R - r;  // rows r .. R-1
#pragma unroll
        for (int j = 0; j < BC_SPT; j++) {
            const int S = S0 + j * BC_THREADS;
            if (S >= nsub) continue;
            double val = 0.0;
            if (__popc(S) <= left) {
                val = Gc[S];
                unsigned cols = (unsigned)S & mk;
                while (cols) {
                    const int c = __ffs(cols) - 1;
                    cols &= cols - 1u;
                    val = val + ar[c] * Gc[S ^ (1 << c)];
                }
            }
            Gn[S] = val;
        }
    }
#pragma unroll
    for (int c = 0; c < BC_MAX; c++)
        if ((mk >> c) & 1u) {  // (uniform)
            const double s = wave_sum63_f64(acc[c]);
            if (lane == 63) red[wave * BC_MAX + c] = s;
        }
    __syncthreads();
    if (tid < m && ((mk >> tid) & 1u)) {
        double s = red[tid];
        for (int w = 1; w < BC_THREADS / 64; w++) s = s + red[w * BC_MAX + tid];
        v.part[((long long)r * v.nwg + wg) * m + tid] = s;
    }
}

// After the sweeps, one workgroup per cluster.  Z' >= KB_RANGE_MIN_Z: the zeros the answer is written over.  Else the complete
// assignments of the pattern are counted, C_{i+1}[S] = C_i[S] + sum_{c in S & N_i} C_i[S \ c] in the two buffers of G: none (and no
// finite entry lost to a' = 0): zeros, log Z = -inf, info 0; else info KB_INFO_OUT_OF_RANGE and nothing else is written.
__global__ void __launch_bounds__(BC_THREADS)
bc_verdict_kernel(BigClusterPack p, const double *sub, double *probs, double *logZ, int *info, double *layers, double *small)
{
    __shared__ int lost;
    const int k = blockIdx.x, tid = threadIdx.x;
    const BcView v = bc_view(p, k, layers, small);
    const int m = v.m, nr = v.rows, R = *v.R, nsub = v.nsub;
    const double Z = v.F[(long long)R * nsub + (nsub - 1)];
    if (!(Z >= KB_RANGE_MIN_Z)) {  // (uniform)
        const double INF = d_inf();
        const double *x = sub + p.c[k].subOff;
        double *cur = v.G, *nxt = v.G + nsub;
        if (tid == 0) lost = 0;
        for (int S = tid; S < nsub; S += BC_THREADS) cur[S] = (S == 0) ? 1.0 : 0.0;
        __syncthreads();
        for (int i = 0; i < R; i++) {
            const unsigned mk = (unsigned)v.mask[i];
            for (int S = tid; S < nsub; S += BC_THREADS) {
                double val = cur[S];
                unsigned cols = (unsigned)S & mk;
                while (cols) {
                    const int c = __ffs(cols) - 1;
                    cols &= cols - 1u;
                    val = val + cur[S ^ (1 << c)];
                }
                nxt[S] = val;
            }
            __syncthreads();
            double *t = cur;
            cur = nxt;
            nxt = t;
        }
        for (int i = tid; i < nr * m; i += BC_THREADS) {  // a finite entry whose a' is 0 took no part in the count
            const double e = x[i];
            if (e < INF && !(exp(v.colMin[i / nr] - e) > 0.0)) lost = 1;
        }
        __syncthreads();
        bool none = R < m;  // fewer rows than columns, or a column without a finite entry: whatever was lost
        for (int c = 0; c < m; c++) none = none | !(v.colMin[c] < INF);
        if (!none && (cur[nsub - 1] > 0.0 || lost)) {
            if (tid == 0 && info) info[p.c[k].idx] = KB_INFO_OUT_OF_RANGE;
            return;
        }
        if (tid == 0) {
            if (logZ) logZ[p.c[k].idx] = -INF;
            if (info) info[p.c[k].idx] = 0;
        }
    }
    double *out = probs + p.c[k].probOff;
    for (int i = tid; i < m * (v.nL + 1); i += BC_THREADS) out[i] = 0.0;
}

// one wave per (row, cluster): lane c sums the partials of column c in ascending workgroup order
__global__ void __launch_bounds__(64)
bc_rows_kernel(BigClusterPack p, double *probs, double *layers, double *small)
{
    const BcView v = bc_view(p, blockIdx.y, layers, small);
    const int R = *v.R, r = blockIdx.x, c = threadIdx.x, m = v.m;
    if (r >= R || c >= m || !(((unsigned)v.mask[r] >> c) & 1u)) return;
    const double Z = v.F[(long long)R * v.nsub + (v.nsub - 1)];
    if (!(Z >= KB_RANGE_MIN_Z)) return;  // (bc_verdict has answered)
    const double *pp = v.part + (long long)r * v.nwg * m + c;
    double s = pp[0];
    for (int w = 1; w < v.nwg; w++) s = s + pp[(long long)w * m];
    const double wv = v.a[r * m + c] * s;
    const int i = v.rowIdx[r];
    if (i < v.nL) probs[p.c[blockIdx.y].probOff + (long long)c * (v.nL + 1) + i] = wv / Z;
    else v.miss[(i - v.nL) * m + c] = wv;
}

__global__ void __launch_bounds__(64)
bc_finish_kernel(BigClusterPack p, double *probs, double *logZ, int *info, double *layers, double *small)
{
    const int k = blockIdx.x, c = threadIdx.x;
    const BcView v = bc_view(p, k, layers, small);
    const int m = v.m;
    const double Z = v.F[(long long)(*v.R) * v.nsub + (v.nsub - 1)];
    const bool ok = Z >= KB_RANGE_MIN_Z;  // (else bc_verdict has answered)
    if (c < m && ok) {  // the rows >= nL_k in ascending order
        double s = v.miss[c];
        for (int t = 1; t < m; t++) s = s + v.miss[t * m + c];
        probs[p.c[k].probOff + (long long)c * (v.nL + 1) + v.nL] = s / Z;
    }
    if (c == 0 && ok) {
        if (logZ) logZ[p.c[k].idx] = log(Z) - *v.sumCol;
        if (info) info[p.c[k].idx] = 1;
    }
}

__global__ void bc_flag_kernel(int *info, int idx, int value) { info[idx] = value; }

}  // namespace

hipError_t launch_bigcluster_pack(const BigClusterPack &p, const double *sub, double *probs, double *logZ, int *info,
                                  double *layers, double *small, hipStream_t stream)
{
    int maxM = 1, maxRows = 0;
    for (int k = 0; k < p.n; k++) {
        if (p.c[k].m > maxM) maxM = p.c[k].m;
        if (p.c[k].rows > maxRows) maxRows = p.c[k].rows;
    }
    const int nsub = 1 << maxM, gx = (nsub + BC_THREADS - 1) / BC_THREADS;
    hipLaunchKernelGGL(bc_setup_kernel, dim3(p.n), dim3(BC_THREADS), 0, stream, p, sub, layers, small);
    hipLaunchKernelGGL(bc_init_kernel, dim3(gx, p.n), dim3(BC_THREADS), 0, stream, p, layers, small);
    for (int i = 0; i < maxRows; i++)
        hipLaunchKernelGGL(bc_forward_kernel, dim3(gx, p.n), dim3(BC_THREADS), 0, stream, p, i, layers, small);
    for (int t = 0; t < maxRows; t++)
        hipLaunchKernelGGL(bc_backward_kernel, dim3(bigcluster_workgroups(maxM), p.n), dim3(BC_THREADS), 0, stream, p, t, layers, small);
    hipLaunchKernelGGL(bc_verdict_kernel, dim3(p.n), dim3(BC_THREADS), 0, stream, p, sub, probs, logZ, info, layers, small);
    if (maxRows > 0) hipLaunchKernelGGL(bc_rows_kernel, dim3(maxRows, p.n), dim3(64), 0, stream, p, probs, layers, small);
    hipLaunchKernelGGL(bc_finish_kernel, dim3(p.n), dim3(64), 0, stream, p, probs, logZ, info, layers, small);
    return hipGetLastError();
}

hipError_t launch_bigcluster_flag(int *info, int idx, int value, hipStream_t stream)
{
    hipLaunchKernelGGL(bc_flag_kernel, dim3(1), dim3(1), 0, stream, info, idx, value);
    return hipGetLastError();
}

}  // namespace kb
