// kbest_hybrid.hip -- the device side of kbest_hybrid_frontier_probs_batch_f64_dev: what hybrid_impl (kbest_capi.cpp) does on the
// host between the partial clustered kernel and the frontier sweep, and after it.  gfx950, plain HIP C++.  DESIGN.md section 15.
//
//   partial kernel (kbest_cluster.hip)     nOpen[B], openDesc[B][maxCol][4], openRows, label, sub, info, logPerm
//   hybrid_gather_kernel                   the open clusters of all frames as ONE list, in frame order, then label order, and
//                                          their count
//   frontier_list_kernel (kbest_frontier.hip)  the sweep over that list: packed probabilities, log Z_k, info, width per cluster
//   hybrid_scatter_kernel                  every taken cluster's [m_k][nL_k + 1] block into its frame; method, nFrontier, logPerm
//
// Stream order between the four launches is the only synchronisation: no workgroup waits for another, there are no atomics, and
// every place in the list follows from a prefix sum over nOpen -- the list, and with it every bit of the outputs, depends on the
// batch alone, not on the grid or on timing.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"

namespace kb {

namespace {

constexpr int HY_THREADS = 256;
constexpr int HY_MAX_COLS = 128;  // KBEST_CLUSTER_MAX_COLS

// a frame's open clusters as the partial kernel counted them (never beyond its descriptors)
__device__ __forceinline__ int hy_open(const HybridParams &p, int b)
{
    const int n = p.nOpen[b];
    return n < 0 ? 0 : n > p.maxCol ? p.maxCol : n;
}

// One thread per frame.  A workgroup first counts the clusters of all frames before its own (integers: any order), then scans its
// own 256 frames; a frame's thread writes the frame's clusters one after another, as the host loop does.
__global__ void __launch_bounds__(HY_THREADS) hybrid_gather_kernel(HybridParams p)
{
    __shared__ int part[HY_THREADS];
    const int tid = threadIdx.x, b0 = blockIdx.x * HY_THREADS, b = b0 + tid;
    int s = 0;
    for (int f = tid; f < b0; f += HY_THREADS) s += hy_open(p, f);
    part[tid] = s;
    __syncthreads();
    for (int h = HY_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    const int base = part[0];
    __syncthreads();
    const int mine = b < p.B ? hy_open(p, b) : 0;
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < HY_THREADS; d <<= 1) {  // inclusive scan
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    if (b >= p.B) return;
    const int at = base + part[tid] - mine;
    p.first[b] = at;
    if (b == p.B - 1) *p.count = at + mine;
    const long long block = ((long long)p.nL[b] + p.nM[b]) * p.nM[b];  // (mine > 0: the partial kernel has checked the frame)
    long long subAt = 0, rowAt = 0, probAt = 0;
    for (int j = 0; j < mine; j++) {
        const int *d = p.openDesc + ((long long)b * p.maxCol + j) * 4;
        const int m = d[1], cL = d[2];
        HybridItem &it = p.list[at + j];
        it.subOff = p.costOff[b] + subAt;
        it.probOff = (long long)b * p.packStride + probAt;
        it.rowAt = (long long)b * p.maxRawRow + rowAt;
        it.b = b;
        it.root = d[0];
        it.m = m;
        it.nL = cL;
        it.idx = at + j;
        const bool sane = m >= 1 && cL >= 0;
        const long long sz = sane ? (long long)(cL + m) * m : 0, pz = sane ? (long long)m * (cL + 1) : 0;
        // more than 64 columns: kept for the scatter's bookkeeping, not sent.  (The other conditions hold for everything the
        // partial kernel writes: a cluster's blocks lie inside its frame's.)
        it.sent = (sane && m <= KB_FRONTIER_MAX_COLS && subAt + sz <= block && probAt + pz <= p.packStride &&
                   rowAt + cL <= p.maxRawRow) ? 1 : 0;
        subAt += sz;
        probAt += pz;
        rowAt += sane ? cL : 0;
    }
}

// One workgroup per frame: the frame's verdict in hybrid_impl's order of precedence, then either zeros or the blocks of its
// clusters, then -- ONE thread, in label order -- logPerm[b] = logPerm[b] + (log Z_k + m_k * mn): the host's expression.
__global__ void __launch_bounds__(HY_THREADS) hybrid_scatter_kernel(HybridParams p)
{
    __shared__ int ctl[2];
    __shared__ int colOf[HY_MAX_COLS];
    __shared__ double waveMin[HY_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double INF = d_inf();
    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        const int nOpen = hy_open(p, b), first = p.first[b], M = p.nM[b], nLo = p.nL[b];
        if (tid == 0) {
            const int info = p.info[b];
            int method = info < 0 ? -1 : info == 0 ? -2 : 0, nFr = 0;
            bool refused = false;
            for (int j = 0; j < nOpen; j++) {
                const int k = first + j;
                if (p.list[k].sent && p.finfo[k] >= 0 && p.width[k] <= p.maxWidth) {
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
        if (nOpen > 0) {  // (uniform; the frame is within the launch bounds: the partial kernel handed clusters out)
            double *fp = p.probs + p.probOff[b];
            if (method < 0) {  // an open cluster without a feasible assignment, or without an answer: the whole frame is zeros
                for (long long i = tid; i < (long long)M * (nLo + 1); i += HY_THREADS) fp[i] = 0.0;
            } else {
                const int *lab = p.label + (long long)b * p.maxCol;
                for (int j = 0; j < nOpen; j++) {
                    const HybridItem it = p.list[first + j];
                    const int m = it.m, cL = it.nL;
                    if (tid < HY_MAX_COLS) colOf[tid] = -1;
                    __syncthreads();
                    for (int c = tid; c < M; c += HY_THREADS)
                        if (lab[c] == it.root) {
                            int rank = 0;
                            for (int e = 0; e < c; e++) rank += (lab[e] == it.root) ? 1 : 0;
                            if (rank < m) colOf[rank] = c;
                        }
                    __syncthreads();
                    // slot nL_k -> slot nL, landmark rows through the row list, columns through the labels
                    const double *q = p.packed + it.probOff;
                    const int *rows = p.openRows + it.rowAt;
                    for (int i = tid; i < m * (cL + 1); i += HY_THREADS) {
                        const int e = i / (cL + 1), r = i - e * (cL + 1), c = colOf[e];
                        const int dst = r < cL ? rows[r] : nLo;
                        if (c >= 0 && dst >= 0 && dst <= nLo) fp[(long long)c * (nLo + 1) + dst] = q[i];
                    }
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
                for (long long i = tid; i < cnt; i += HY_THREADS) v = min_keep(v, x[i]);
                v = wave_min_f64(v);
                if (lane == 0) waveMin[wave] = v;
                __syncthreads();
                mn = waveMin[0];
                for (int w = 1; w < HY_THREADS / 64; w++) mn = min_keep(mn, waveMin[w]);
            }
            if (tid == 0) {
                double lp = p.logPerm[b];
                if (method >= 0)
                    for (int j = 0; j < nOpen; j++) lp = lp + (p.logZ[first + j] + (double)p.list[first + j].m * mn);
                if (method == -2) lp = -INF;
                if (method == -1) lp = __longlong_as_double(0x7ff8000000000000LL);
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

hipError_t launch_hybrid_gather(const HybridParams &p, hipStream_t stream)
{
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_gather_kernel, dim3((p.B + HY_THREADS - 1) / HY_THREADS), dim3(HY_THREADS), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_hybrid_scatter(const HybridParams &p, hipStream_t stream)
{
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(hybrid_scatter_kernel, dim3(p.B < 4096 ? p.B : 4096), dim3(HY_THREADS), 0, stream, p);
    return hipGetLastError();
}

}  // namespace kb
