// kbest_hybrid_sample.hip -- the device side of kbest_hybrid_frontier_sample_assoc_batch_f64_dev: what the host entry
// kbest_hybrid_frontier_sample_assoc_batch_f64 (kbest_capi.cpp) does between its kernels, and after them.  gfx950, plain HIP C++.
// DESIGN.md section 19.
//
//   hybrid_sample_prepare_kernel               where the partial kernel's probabilities go: a packed scratch nobody reads
//   partial kernel (kbest_cluster.hip)         nOpen[B], openDesc[B][maxCol][4], openRows, label, sub, info, logPerm
//   clustered sampler, second instantiation    the draws of the clusters of at most maxExact columns, straight into the caller's
//   (kbest_cluster_sample_partial.hip)         assign and logProb; the open clusters' columns -1
//   hybrid_gather_kernel (kbest_hybrid.hip)    the open clusters of all frames as ONE list, frame order, then label order
//   hybrid_sample_keys_kernel                  per cluster of that list: the keys q of its rows (the RAW rows of the caller's
//                                              block), where its local draws and its terms go, its frame's key
//   frontier_sample_list_kernel                the sampler of kbest_frontier_sample.hip over the list, ONE launch
//   hybrid_sample_join_kernel                  method, nFrontier; the open clusters' columns and terms into the frame's draws, in
//                                              label order; logPerm
//
// Stream order between the launches is the only synchronisation: no workgroup waits for another, there are no atomics, every
// place follows from the frame index and a prefix sum.  A sum of doubles is either one thread's (logPerm, in label order) or one
// addition per cluster in label order by the draw's own thread (logProb): the host's expressions, the host's bits.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"

namespace kb {

namespace {

constexpr int HS_THREADS = 256;
constexpr int HS_MAX_COLS = 128;   // KBEST_CLUSTER_MAX_COLS
constexpr int HS_MAX_ROWS = 1024;  // KBEST_MAX_DIM_WIDE

// a frame's open clusters as the partial kernel counted them (never beyond its descriptors)
__device__ __forceinline__ int hs_open(const HybridSampleParams &p, int b)
{
    const int n = p.nOpen[b];
    return n < 0 ? 0 : n > p.maxCol ? p.maxCol : n;
}

// somebody took cluster k of the list: hybrid_scatter_kernel's condition; maxWidth = 0 sends nothing through the sampler
__device__ __forceinline__ bool hs_taken(const HybridSampleParams &p, int k)
{
    return p.maxWidth > 0 && p.keys[k].sent && p.finfo[k] >= 0 && p.width[k] <= p.maxWidth;
}

__global__ void __launch_bounds__(HS_THREADS) hybrid_sample_prepare_kernel(HybridSampleParams p)
{
    const int b = blockIdx.x * HS_THREADS + threadIdx.x;
    if (b < p.B) p.probOff[b] = (long long)b * p.packStride;
}

// One workgroup per frame with open clusters.  The gate is kbest_cluster.hip's (conditionCosts, the block minimum, 42) with
// comparisons and differences alone -- FrameGate of kbest_capi.cpp: column minima, value(c, r) = x - colMin_c where
// x <= colMin_c + 42 (else +inf) when conditioning, the rows kept (one value < +inf), mn over the kept rows, and
// nonzero(c, r) = kept[r] && mn + 42 > value(c, r).  A row that is not kept holds +inf alone, so mn needs no second pass.
__global__ void __launch_bounds__(HS_THREADS) hybrid_sample_keys_kernel(HybridSampleParams p)
{
    __shared__ double colMin[HS_MAX_COLS];
    __shared__ double waveMin[HS_THREADS / 64];
    __shared__ u64 bal[HS_THREADS / 64];
    __shared__ int lab[HS_MAX_COLS];
    __shared__ unsigned char kept[HS_MAX_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = d_inf();
    const bool cond = p.condition != 0;
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int nOpen = hs_open(p, b);
        if (nOpen == 0) continue;  // (uniform)
        const int M = p.nM[b], nLo = p.nL[b], NR = nLo + M, first = p.first[b];
        const u64 frameKey = p.frameKey ? p.frameKey[b] : (u64)b;
        if (M < 1 || M > HS_MAX_COLS || nLo < 0 || NR > HS_MAX_ROWS) {  // (never: the partial kernel hands nothing out there)
            for (int j = tid; j < nOpen; j += HS_THREADS) p.keys[first + j] = HybridKeyItem{0, 0, 0, frameKey, 0, 0};
            continue;
        }
        const double *x = p.cost + p.costOff[b];
        if (tid < M) lab[tid] = p.label[(long long)b * p.maxCol + tid];
        if (cond)
            for (int c = wave; c < M; c += HS_THREADS / 64) {  // a wave per column: the reads along r are contiguous
                double v = INF;
                for (int r = lane; r < NR; r += 64) v = min_keep(v, x[(long long)c * NR + r]);
                v = wave_min_f64(v);
                if (lane == 0) colMin[c] = v;
            }
        __syncthreads();
        double v = INF;
        for (int r = tid; r < NR; r += HS_THREADS) {
            bool good = !cond;
            for (int c = 0; c < M; c++) {
                const double e = x[(long long)c * NR + r];
                if (cond) {
                    const bool in = e <= colMin[c] + 42.0;
                    good = good | in;
                    v = min_keep(v, in ? e - colMin[c] : INF);
                } else {
                    v = min_keep(v, e);
                }
            }
            kept[r] = good ? 1 : 0;
        }
        v = wave_min_f64(v);
        if (lane == 0) waveMin[wave] = v;
        __syncthreads();
        double mn = waveMin[0];
        for (int w = 1; w < HS_THREADS / 64; w++) mn = min_keep(mn, waveMin[w]);
        // the clusters one after another, as the host loop: every running sum is uniform over the workgroup
        int keyAt = 0, asgAt = 0;
        for (int j = 0; j < nOpen; j++) {
            const int k = first + j;
            const HybridItem it = p.list[k];
            const int m = it.m, cL = it.nL, R = p.openDesc[((long long)b * p.maxCol + j) * 4 + 3];
            bool sent = it.sent && R >= cL && R - cL <= m && keyAt + cL + m <= p.maxRawRow && asgAt + m <= p.maxCol;
            if (sent) {  // (uniform)
                int *key = p.rowKey + (long long)b * p.maxRawRow + keyAt;
                const int *rows = p.openRows + it.rowAt;
                for (int r = tid; r < cL; r += HS_THREADS) key[r] = rows[r];
                // thread t: the miss row nL + t.  The rows of the cluster, ascending: a ballot and the bits below
                bool mine = false;
                if (tid < M && kept[nLo + tid]) {
                    const int r = nLo + tid;
                    for (int c = 0; c < M; c++) {
                        double e = x[(long long)c * NR + r];
                        if (cond) e = (e <= colMin[c] + 42.0) ? (e - colMin[c]) : INF;
                        mine = mine | (lab[c] == it.root && mn + 42.0 > e);
                    }
                }
                const u64 mask = __ballot(mine);
                if (lane == 0) bal[wave] = mask;
                __syncthreads();
                const int found = __popcll(bal[0]) + __popcll(bal[1]);  // (M <= 128: waves 0 and 1)
                const int rank = (wave == 0 ? 0 : __popcll(bal[0])) + __popcll(mask & ((1ull << lane) - 1ull));
                if (mine && rank < m) key[cL + rank] = nLo + tid;
                sent = found == R - cL;  // (the host entry: KBEST_ERR_INTERNAL)
                if (sent)
                    for (int r = R + tid; r < cL + m; r += HS_THREADS) key[r] = 0;  // all-+inf rows: no steps
            }
            if (tid == 0)
                p.keys[k] = HybridKeyItem{(long long)b * p.maxRawRow + keyAt, ((long long)b * p.maxCol + asgAt) * p.nSample,
                                          (long long)k * p.nSample, frameKey, R, sent ? 1 : 0};
            if (sent) {
                keyAt += cL + m;
                asgAt += m;
            }
            __syncthreads();  // (bal: the next cluster's)
        }
    }
}

// One workgroup per frame: the frame's verdict in the host entry's order of precedence (hybrid_scatter_kernel's), then either
// -1s and NaNs or the open clusters' columns and terms, cluster after cluster in label order -- thread t owns the draws
// t, t + 256, ...: logProb[s] = logProb[s] + term[s] is one addition per cluster by one thread.  Then -- ONE thread, in label
// order -- logPerm = (the partial kernel's sum) + (log Z_k + m_k * mn) ...: the host's expression.
__global__ void __launch_bounds__(HS_THREADS) hybrid_sample_join_kernel(HybridSampleParams p)
{
    __shared__ int ctl[2];
    __shared__ int colOf[HS_MAX_COLS];
    __shared__ double waveMin[HS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = d_inf();
    const double QNAN = __longlong_as_double(0x7ff8000000000000LL);
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int nOpen = hs_open(p, b), first = p.first[b], M = p.nM[b], nLo = p.nL[b];
        if (tid == 0) {
            const int info = p.info[b];
            int method = info < 0 ? -1 : info == 0 ? -2 : 0, nFr = 0;
            bool refused = false;
            for (int j = 0; j < nOpen; j++) {
                const int k = first + j;
                if (hs_taken(p, k)) {
                    if (p.finfo[k] <= 0) method = -2;
                    else nFr++;
                } else {
                    refused = true;  // nobody took it
                }
            }
            if (refused) method = -1;
            if (method < 0 && nOpen > 0) nFr = 0;
            ctl[0] = method;
            ctl[1] = nFr;
        }
        __syncthreads();
        const int method = ctl[0];
        const bool within = !(M < 1 || M > p.maxCol || nLo < 0 || nLo + M > p.maxRawRow);  // (uniform) the launch bounds
        if (within) {
            int *fa = p.assign + p.asgOff[b];
            double *fl = p.logProb + p.lpOff[b];
            if (method != 0) {
                for (long long i = tid; i < (long long)p.nSample * M; i += HS_THREADS) fa[i] = -1;
                for (int s = tid; s < p.nSample; s += HS_THREADS) fl[s] = QNAN;
            } else {
                const int *lab = p.label + (long long)b * p.maxCol;
                for (int j = 0; j < nOpen; j++) {
                    const HybridItem it = p.list[first + j];
                    const HybridKeyItem ky = p.keys[first + j];
                    const int m = it.m, R = ky.R;
                    if (tid < HS_MAX_COLS) colOf[tid] = -1;
                    __syncthreads();
                    for (int c = tid; c < M; c += HS_THREADS)
                        if (lab[c] == it.root) {
                            int rank = 0;
                            for (int e = 0; e < c; e++) rank += (lab[e] == it.root) ? 1 : 0;
                            if (rank < m) colOf[rank] = c;
                        }
                    __syncthreads();
                    // local rows back to raw rows through the keys, columns through the labels
                    const int *key = p.rowKey + ky.rowKeyOff, *loc = p.local + ky.asgOff;
                    const double *term = p.term + ky.ltOff;
                    for (long long i = tid; i < (long long)p.nSample * m; i += HS_THREADS) {
                        const long long s = i / m;
                        const int e = (int)(i - s * m), r = loc[i], c = colOf[e];
                        if (c >= 0) fa[s * M + c] = (r >= 0 && r < R) ? key[r] : -1;
                    }
                    for (int s = tid; s < p.nSample; s += HS_THREADS) fl[s] = fl[s] + term[s];
                    __syncthreads();
                }
            }
        }
        if (p.logPerm) {
            double mn = 0.0;
            if (!p.condition && method >= 0 && nOpen > 0) {  // (uniform) the frame's block minimum
                const double *x = p.cost + p.costOff[b];
                const long long cnt = ((long long)nLo + M) * M;
                double v = INF;
                for (long long i = tid; i < cnt; i += HS_THREADS) v = min_keep(v, x[i]);
                v = wave_min_f64(v);
                if (lane == 0) waveMin[wave] = v;
                __syncthreads();
                mn = waveMin[0];
                for (int w = 1; w < HS_THREADS / 64; w++) mn = min_keep(mn, waveMin[w]);
            }
            if (tid == 0) {
                // a frame without an open cluster: the sampler's own sum.  Else the partial kernel's, then the open clusters
                double lp = !within ? QNAN : nOpen > 0 ? p.partLogPerm[b] : p.drawLogPerm[b];
                if (method >= 0)
                    for (int j = 0; j < nOpen; j++) lp = lp + (p.logZ[first + j] + (double)p.list[first + j].m * mn);
                if (method == -2) lp = -INF;
                if (method == -1) lp = QNAN;
                p.logPerm[b] = lp;
            }
        }
        if (tid == 0) {
            p.method[b] = method;
            if (p.nFrontier) p.nFrontier[b] = ctl[1];
            if (p.nOpenOut) p.nOpenOut[b] = p.nOpen[b];
        }
        __syncthreads();  // (ctl, waveMin: the next frame's)
    }
}

}  // namespace

hipError_t launch_hybrid_sample_prepare(const HybridSampleParams &p, hipStream_t stream)
{
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_sample_prepare_kernel, dim3((p.B + HS_THREADS - 1) / HS_THREADS), dim3(HS_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_hybrid_sample_keys(const HybridSampleParams &p, hipStream_t stream)
{
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_sample_keys_kernel, dim3(p.B < 4096 ? p.B : 4096), dim3(HS_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_hybrid_sample_join(const HybridSampleParams &p, hipStream_t stream)
{
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_sample_join_kernel, dim3(p.B < 4096 ? p.B : 4096), dim3(HS_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace kb
