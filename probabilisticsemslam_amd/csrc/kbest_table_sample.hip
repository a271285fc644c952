// kbest_table_sample.hip -- joint associations DRAWN from a table of k best assignments, under the weights assignmentProb
// (assignment.cpp:616-648) gives its slots: the draws of a cluster that no exact tier takes.  One workgroup of 256 per problem, one
// launch per pack of problems, the grid strides over the pack.  gfx950, fp64, plain HIP C++.  DESIGN.md section 20.
//
// Input: what kbest_batch_f64_dev writes -- row4col [n][k][maxCol] int32, gain [n][k] double (ascending), nf [n] int32.  Per problem
// (kbest_table_sample.h has every expression; a host program runs the same lines):
//     w_j = exp(gain_0 - gain_j) where gain_0 + cutoff > gain_j, else 0        all threads, into LDS
//     P_j = P_{j-1} + w_j from 0.0, j ascending; total = P_{nf-1}               ONE thread, in place: the order is the contract
//     draw s: T = u total, the first j with T < P_j by bisection (if rounding leaves none: the last j with w_j > 0)
//     logTerm[s] = (gain_0 - gain_j) - log(total);  pick[s] = j;  assignLocal[s][c] = row4col[j][c], c < m
// The draws go in rounds of 256: a thread finds the slot of its draw and leaves it in LDS, then the workgroup copies the rounds'
// rows together, consecutive threads on consecutive words.  The uniform: Philox4x32-10, key (seed low, seed high), counter
// (sampleBase + s, 0x40000000 | clusterKey, frameKey low, frameKey high), words 0 and 1: bit 30 set and bit 31 clear keeps these
// uniforms apart from kbest_cluster_sample.hip's (second word <= 511) and from kbest_frontier_sample.hip's (bit 31 set).
// info: 1 drawn; 0 (nf <= 0, or no slot with a weight > 0): assignLocal -1, logTerm NaN, pick -1; -1 (m outside 1 .. maxCol):
// nothing is touched.  No workgroup waits for another, no floating-point atomics, no sum over threads, every loop has a bound: a
// problem's outputs are a function of (table, cutoff, seed, keys, draw index) alone, anywhere in a batch.
#include <hip/hip_runtime.h>

#include "kbest_table_sample.h"

namespace kb {

namespace {

__global__ void __launch_bounds__(TS_THREADS)
table_sample_kernel(TableSamplePack p, int k, int maxCol, const int *row4col, const double *gain, const int *nf, double cutoff,
                    int nSample, unsigned long long seed, unsigned sampleBase, int *assignLocal, double *logTerm, int *pick, int *info)
{
    __shared__ double P[TS_MAX_K];
    __shared__ int slot[TS_THREADS];
    __shared__ int sLast;
    const int tid = threadIdx.x;
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const double QNAN = __builtin_nan("");
    for (int q = blockIdx.x; q < p.n; q += gridDim.x) {
        const TableSampleDesc &d = p.c[q];
        const int idx = p.base + q, m = d.m;
        if (m < 1 || m > maxCol) {  // (uniform: the whole workgroup leaves the problem)
            if (tid == 0 && info) info[idx] = -1;
            continue;
        }
        int n = nf[idx];
        if (n > k) n = k;
        int *asg = assignLocal + d.asgOff, *pk = pick ? pick + (long long)idx * nSample : nullptr;
        double *lt = logTerm + d.ltOff;
        const double *g = gain + (long long)idx * k;
        const int *tab = row4col + (long long)idx * k * maxCol;
        const double g0 = n > 0 ? g[0] : 0.0;
        __syncthreads();  // (the problem before this one is done with P)
        for (int j = tid; j < n; j += TS_THREADS) P[j] = ts_weight(g0, g[j], cutoff);
        __syncthreads();
        if (tid == 0) sLast = ts_accumulate(P, n);
        __syncthreads();
        const int last = sLast;
        const long long cells = (long long)nSample * m;
        if (last < 0) {  // nothing to draw from
            for (long long e = tid; e < cells; e += TS_THREADS) asg[e] = -1;
            for (int s = tid; s < nSample; s += TS_THREADS) {
                lt[s] = QNAN;
                if (pk) pk[s] = -1;
            }
            if (tid == 0 && info) info[idx] = 0;
            continue;
        }
        const double total = P[n - 1], logTotal = log(total);
        const unsigned f0 = (unsigned)d.frameKey, f1 = (unsigned)(d.frameKey >> 32);
        for (int s0 = 0; s0 < nSample; s0 += TS_THREADS) {
            const int s = s0 + tid, cnt = nSample - s0 < TS_THREADS ? nSample - s0 : TS_THREADS;
            if (s < nSample) {
                const double T = ts_uniform(sampleBase + (unsigned)s, d.clusterKey, f0, f1, k0, k1) * total;
                const int j = ts_pick(P, n, last, T);
                slot[tid] = j;
                lt[s] = ts_log_term(g0, g[j], logTotal);
                if (pk) pk[s] = j;
            }
            __syncthreads();
            int *out = asg + (long long)s0 * m;
            for (int e = tid; e < cnt * m; e += TS_THREADS) {  // (cnt * m <= 256 maxCol)
                const int sl = e / m, c = e - sl * m;
                out[e] = tab[(long long)slot[sl] * maxCol + c];
            }
            __syncthreads();  // (slot is free again)
        }
        if (tid == 0 && info) info[idx] = 1;
    }
}

}  // namespace

int launch_table_sample_pack(const TableSamplePack &p, int k, int maxCol, const int *row4col, const double *gain, const int *nf,
                             double cutoff, int nSample, unsigned long long seed, unsigned sampleBase, int *assignLocal,
                             double *logTerm, int *pick, int *info, void *stream)
{
    if (p.n <= 0) return (int)hipSuccess;
    hipLaunchKernelGGL(table_sample_kernel, dim3(p.n), dim3(TS_THREADS), 0, static_cast<hipStream_t>(stream), p, k, maxCol, row4col,
                       gain, nf, cutoff, nSample, seed, sampleBase, assignLocal, logTerm, pick, info);
    return (int)hipGetLastError();
}

}  // namespace kb
