// kbest_table_sample.h -- the parts of kbest_table_sample.hip that are plain C++: the uniform of a draw, the weight of one slot of a
// table of k best assignments, the running sums P, the pick and the log term; and what the kernel's launcher takes.  __host__
// __device__, no HIP type: tests/cpp/table_sample_host.cpp includes this file alone (after <cmath>) and runs it under sanitizers on
// exact-size heap blocks.  The distribution is assignmentProb's (assignment.cpp:616-648) over the table kbest_batch_f64_dev writes:
//     w_j = exp(gain_0 - gain_j) where gain_0 + cutoff > gain_j (strictly), else 0;  P_j = P_{j-1} + w_j from 0.0, left to right;
//     total = P_{nf-1};  a draw with T = u total takes the FIRST j with T < P_j, and the last j with w_j > 0 if rounding leaves none.
#ifndef KBEST_TABLE_SAMPLE_H
#define KBEST_TABLE_SAMPLE_H

#include "kbest_cluster_sample.h"

namespace kb {

constexpr int TS_MAX_K = 4096;                 // KBEST_TABLE_SAMPLE_MAX_K: P of one problem in LDS, 32 KiB
constexpr int TS_THREADS = 256;
constexpr unsigned TS_DOMAIN = 0x40000000u;    // bit 30 of the counter's second word: the table sampler's uniforms
constexpr unsigned TS_MAX_KEY = 0x40000000u;   // clusterKey < 2^30

// u of draw (sampleBase + s) on the cluster with key clusterKey (< 2^30) of the frame with key (f0, f1): Philox4x32-10, key (seed
// low, seed high), counter (draw, 0x40000000 | clusterKey, f0, f1), words 0 and 1
__host__ __device__ inline double ts_uniform(unsigned draw, unsigned clusterKey, unsigned f0, unsigned f1, unsigned k0, unsigned k1)
{
    const CsPhilox rnd = cs_philox4x32_10(draw, TS_DOMAIN | clusterKey, f0, f1, k0, k1);
    return (double)((((unsigned long long)rnd.w[1] << 32) | rnd.w[0]) >> 11) * 0x1.0p-53;
}

// the weight of a slot with gain gj in a table whose first gain is g0 (a slot at or beyond the cutoff, or a NaN: 0)
__host__ __device__ inline double ts_weight(double g0, double gj, double cutoff) { return (g0 + cutoff > gj) ? exp(g0 - gj) : 0.0; }

// P[0 .. nf-1]: the weights in, their running sums out (one addition per slot, from 0.0, in table order).  Returns the last slot
// whose weight was > 0, or -1.
__host__ __device__ inline int ts_accumulate(double *P, int nf)
{
    double acc = 0.0;
    int last = -1;
    for (int j = 0; j < nf; j++) {
        const double w = P[j];
        if (w > 0.0) last = j;
        acc = acc + w;
        P[j] = acc;
    }
    return last;
}

// the first j of 0 .. nf-1 with T < P[j] (P does not decrease: a bisection gives the index of the linear scan; at most 13 steps
// for nf <= 4096), else `last`
__host__ __device__ inline int ts_pick(const double *P, int nf, int last, double T)
{
    int lo = 0, hi = nf;  // the answer lies in [lo, hi]; hi = nf: none
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (T < P[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo < nf ? lo : last;
}

// the log-probability of slot j under the table's weights: no log of a product
__host__ __device__ inline double ts_log_term(double g0, double gj, double logTotal) { return (g0 - gj) - logTotal; }

// ---- the launcher of kbest_table_sample.hip: the problems of a launch travel as a kernel argument, nothing is staged or allocated ---
constexpr int KB_TABLE_SAMPLE_PACK = 64;       // problems of one launch
struct TableSampleDesc {
    long long asgOff, ltOff;            // its [nSample][m] rows / its [nSample] terms, from the caller's buffers
    unsigned long long frameKey;        // words 2 and 3 of the generator's counter
    unsigned clusterKey;                // < 2^30: the low bits of word 1
    int m;                              // columns of the problem
};
struct TableSamplePack {
    TableSampleDesc c[KB_TABLE_SAMPLE_PACK];
    int n, base;                        // problems; the place of the first one in the tables, in pick and in info
};
// stream: a hipStream_t.  Returns a hipError_t.
int launch_table_sample_pack(const TableSamplePack &p, int k, int maxCol, const int *row4col, const double *gain, const int *nf,
                             double cutoff, int nSample, unsigned long long seed, unsigned sampleBase, int *assignLocal,
                             double *logTerm, int *pick, int *info, void *stream);

}  // namespace kb
#endif
