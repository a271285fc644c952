// kbest_quadric_map.hip -- computeQuadricCostMatrix and conditionCosts (assignment.cpp:705-722, :450-494) in one go for a frame
// against a map of any size: the raw (nL + nM) x nM block is never written.  A landmark row survives conditionCosts only if some
// column has cost <= colMin[c] + 42, and colMin[c] <= gate (the column's dummy row), so of thousands of landmarks a few dozen
// remain; the kernels here find them and write the compact conditioned block -- kept landmark rows in ascending order, then all
// nM dummy rows -- that the one-stream exact path (kbest_hybrid_frontier_probs_batch_f64_dev, condition = 0) takes.
//
//   qmap_min_kernel    one thread per landmark row, QMAP_TILE rows a workgroup: the costs of the row against every measurement
//                      (the frame's measurements in LDS, the landmark in registers), per column the wave minimum, then the
//                      minimum over the workgroup's waves in wave order -> tileMin
//   qmap_colmin_kernel folds a frame's tile minima in tile order, then the gate -> colMin
//   qmap_flag_kernel   the costs again; a row is kept if some column has cost <= colMin + 42; the ballot of each wave -> keep,
//                      the workgroup's count -> tileCnt
//   qmap_scan_kernel   exclusive prefix sum of a frame's tile counts -> tileOff, nKeep; the offsets of the frame's compact
//                      block and compact probabilities
//   qmap_rows_kernel   rowIdx[tileOff + rank within the tile] = row, from the ballots
//   qmap_fill_kernel   one thread per kept row: its costs a third time, conditioned, into the compact block; the dummy rows
//   qmap_expand_kernel the dense [nM][nL + 1] slice from the compact [nM][nKeep + 1] one: every element written once
//
// The cost is recomputed rather than stored.  No floating-point atomics, no workgroup waits for another: stream order between the
// launches is the only synchronisation.  A minimum is the leftmost smallest entry in row order whatever the tile size -- waves are
// 64 consecutive rows from row 0 of the frame, and "leftmost minimum" is associative -- so a frame's outputs do not depend on the
// batch, the tile size or the bounds of the launch.  A NaN cost (singular S) never passes `<=`: it counts as +inf in the minima.
// Every row number is an int32 below KBEST_QUADRIC_MAP_MAX = 2^22; every index into the map and the buffers is 64-bit.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_wave.h"
#include "kbest_quadric.h"
#include "kbest_quadric_map.h"

namespace kb {

__device__ __forceinline__ double qmap_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// the cost of quadric_cost_kernel (kbest_costs.hip), operation for operation
__device__ __forceinline__ double qmap_cost(const double *m1, const double *c1, const double *m2, const double *c2)
{
    double d[3], S[9], x[3];
#pragma unroll
    for (int j = 0; j < 3; j++) d[j] = m1[j] - m2[j];
#pragma unroll
    for (int j = 0; j < 9; j++) S[j] = c1[j] + c2[j];
    ldlt3_solve(S, d, x);
    return d[0] * x[0] + d[1] * x[1] + d[2] * x[2];
}

// A frame the launch takes: 1 <= nM <= maxCol, 0 <= nL <= maxMap, no negative offset.  Uniform over a workgroup.
__device__ __forceinline__ bool qmap_frame(const QuadricMapParams &p, int b, int &nL, int &nM)
{
    nL = p.nL[b];
    nM = p.nM[b];
    return nM >= 1 && nM <= p.maxCol && nL >= 0 && nL <= p.maxMap && p.landOff[b] >= 0 && p.measOff[b] >= 0;
}

// the frame's measurements into LDS: means at sMeas[c * 12 .. + 3), covariances at sMeas[c * 12 + 3 .. + 12)
__device__ __forceinline__ void qmap_load_meas(const QuadricMapParams &p, int b, int nM, double *sMeas)
{
    const double *mm = p.measMean + 3 * p.measOff[b], *mc = p.measCov + 9 * p.measOff[b];
    for (int i = threadIdx.x; i < nM * 12; i += QMAP_TILE) {
        const int c = i / 12, j = i - c * 12;
        sMeas[i] = j < 3 ? mm[(long long)c * 3 + j] : mc[(long long)c * 9 + (j - 3)];
    }
}

__device__ __forceinline__ void qmap_load_land(const QuadricMapParams &p, int b, int r, double *m1, double *c1)
{
    const long long at = p.landOff[b] + (long long)r;
#pragma unroll
    for (int j = 0; j < 3; j++) m1[j] = p.mapMean[at * 3 + j];
#pragma unroll
    for (int j = 0; j < 9; j++) c1[j] = p.mapCov[at * 9 + j];
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_min_kernel(QuadricMapParams p)
{
    __shared__ double sMeas[12 * QMAP_MAX_COLS];
    __shared__ double sMin[QMAP_TILE / 64][QMAP_MAX_COLS];
    const int b = blockIdx.x / p.nTiles, tile = blockIdx.x - b * p.nTiles, tid = threadIdx.x;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM) || tile * QMAP_TILE >= nL) return;
    qmap_load_meas(p, b, nM, sMeas);
    const int r = tile * QMAP_TILE + tid;
    const bool valid = r < nL;
    double m1[3] = {0, 0, 0}, c1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (valid) qmap_load_land(p, b, r, m1, c1);
    __syncthreads();
    for (int c = 0; c < nM; c++) {
        double v = qmap_inf();
        if (valid) {
            v = qmap_cost(m1, c1, sMeas + c * 12, sMeas + c * 12 + 3);
            if (v != v) v = qmap_inf();
        }
        const double wm = wave_min_f64(v);
        if ((tid & 63) == 0) sMin[tid >> 6][c] = wm;
    }
    __syncthreads();
    for (int c = tid; c < nM; c += QMAP_TILE) {
        double m = sMin[0][c];
        for (int w = 1; w < QMAP_TILE / 64; w++) m = min_keep(m, sMin[w][c]);
        p.tileMin[(long long)blockIdx.x * p.maxCol + c] = m;
    }
}

// (:450-458: colMins starts at +inf and moves on where an entry compares less; the column's own dummy row comes last)
__global__ void __launch_bounds__(QMAP_MAX_COLS) qmap_colmin_kernel(QuadricMapParams p)
{
    const int b = blockIdx.x, c = threadIdx.x;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM) || c >= nM) return;
    const int nt = (nL + QMAP_TILE - 1) / QMAP_TILE;
    double m = qmap_inf();
    for (int t = 0; t < nt; t++) m = min_keep(m, p.tileMin[((long long)b * p.nTiles + t) * p.maxCol + c]);
    p.colMin[(long long)b * p.maxCol + c] = min_keep(m, p.gate);
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_flag_kernel(QuadricMapParams p)
{
    __shared__ double sMeas[12 * QMAP_MAX_COLS];
    __shared__ double sCut[QMAP_MAX_COLS];
    __shared__ int sCnt[QMAP_TILE / 64];
    const int b = blockIdx.x / p.nTiles, tile = blockIdx.x - b * p.nTiles, tid = threadIdx.x;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM) || tile * QMAP_TILE >= nL) return;
    qmap_load_meas(p, b, nM, sMeas);
    for (int c = tid; c < nM; c += QMAP_TILE) sCut[c] = p.colMin[(long long)b * p.maxCol + c] + 42.0;  // (:468: colMins[col] + cutoff)
    const int r = tile * QMAP_TILE + tid;
    const bool valid = r < nL;
    double m1[3] = {0, 0, 0}, c1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (valid) qmap_load_land(p, b, r, m1, c1);
    __syncthreads();
    bool good = false;
    if (valid)
        for (int c = 0; c < nM; c++) good = good || qmap_cost(m1, c1, sMeas + c * 12, sMeas + c * 12 + 3) <= sCut[c];
    const u64 mask = __ballot(good);
    if ((tid & 63) == 0) {
        p.keep[(long long)blockIdx.x * (QMAP_TILE / 64) + (tid >> 6)] = mask;
        sCnt[tid >> 6] = __popcll(mask);
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int w = 0; w < QMAP_TILE / 64; w++) n += sCnt[w];
        p.tileCnt[blockIdx.x] = n;
    }
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_scan_kernel(QuadricMapParams p)
{
    __shared__ int sSum[QMAP_TILE];
    const int b = blockIdx.x, tid = threadIdx.x;
    int nL, nM;
    const bool ok = qmap_frame(p, b, nL, nM);
    if (tid == 0) {  // where the frame's compact block and compact probabilities lie: the same for every frame of the launch
        p.costOff[b] = (long long)b * (p.maxKeep + p.maxCol) * p.maxCol;
        p.cprobOff[b] = (long long)b * p.maxCol * (p.maxKeep + 1);
        if (!ok) p.nLh[b] = -1;
    }
    if (!ok) return;
    const int nt = (nL + QMAP_TILE - 1) / QMAP_TILE, per = (nt + QMAP_TILE - 1) / QMAP_TILE;
    const int lo = tid * per < nt ? tid * per : nt, hi = lo + per < nt ? lo + per : nt;
    const long long base = (long long)b * p.nTiles;
    int s = 0;
    for (int t = lo; t < hi; t++) s += p.tileCnt[base + t];
    sSum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < QMAP_TILE; i++) { const int v = sSum[i]; sSum[i] = run; run += v; }
        p.nKeep[b] = run;                        // the TRUE count, also beyond maxKeep
        p.nLh[b] = run <= p.maxKeep ? run : -1;  // beyond: the exact path refuses the frame (method -1) and touches nothing
    }
    __syncthreads();
    int off = sSum[tid];
    for (int t = lo; t < hi; t++) { p.tileOff[base + t] = off; off += p.tileCnt[base + t]; }
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_rows_kernel(QuadricMapParams p)
{
    const int b = blockIdx.x / p.nTiles, tile = blockIdx.x - b * p.nTiles, tid = threadIdx.x;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM) || tile * QMAP_TILE >= nL || p.nLh[b] < 0) return;
    const int w = tid >> 6, lane = tid & 63;
    int at = p.tileOff[blockIdx.x];
    for (int i = 0; i < w; i++) at += __popcll(p.keep[(long long)blockIdx.x * (QMAP_TILE / 64) + i]);
    const u64 mask = p.keep[(long long)blockIdx.x * (QMAP_TILE / 64) + w];
    if ((mask >> lane) & 1) {
        at += __popcll(mask & ((1ull << lane) - 1));
        if (at < p.maxKeep) p.rowIdx[(long long)b * p.maxKeep + at] = tile * QMAP_TILE + tid;  // (at < nKeep <= maxKeep: checked all the same)
    }
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_fill_kernel(QuadricMapParams p)
{
    __shared__ double sMeas[12 * QMAP_MAX_COLS];
    __shared__ double sMin[QMAP_MAX_COLS];
    const int b = blockIdx.x / p.nKeepTiles, j = blockIdx.x - b * p.nKeepTiles, tid = threadIdx.x;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM)) return;
    const int nk = p.nLh[b];
    if (nk < 0 || (j > 0 && j * QMAP_TILE >= nk)) return;
    qmap_load_meas(p, b, nM, sMeas);
    for (int c = tid; c < nM; c += QMAP_TILE) sMin[c] = p.colMin[(long long)b * p.maxCol + c];
    __syncthreads();
    const long long nR = (long long)nk + nM;
    double *out = p.ccost + p.costOff[b];
    const int s = j * QMAP_TILE + tid;
    if (s < nk) {
        const int r = p.rowIdx[(long long)b * p.maxKeep + s];
        if (r >= 0 && r < nL) {
            double m1[3], c1[9];
            qmap_load_land(p, b, r, m1, c1);
            for (int c = 0; c < nM; c++) {
                const double x = qmap_cost(m1, c1, sMeas + c * 12, sMeas + c * 12 + 3);
                out[c * nR + s] = x <= sMin[c] + 42.0 ? x - sMin[c] : qmap_inf();  // (:490-491)
            }
        }
    }
    if (j == 0)  // the dummy rows, all nM of them: the gate on each column's own, +inf elsewhere (:713-720), conditioned alike
        for (int i = tid; i < nM * nM; i += QMAP_TILE) {
            const int c = i / nM, q = i - c * nM;
            double v = qmap_inf();
            if (q == c && p.gate <= sMin[c] + 42.0) v = p.gate - sMin[c];
            out[c * nR + nk + q] = v;
        }
}

// probs[m][rowIdx[l]] = cprobs[m][l], probs[m][nL] = cprobs[m][nKeep], every other element 0.0 (rowIdx ascends: a binary search
// tells whether a landmark was kept).  A frame over maxKeep: zeros.  A frame the launch does not take: untouched.
__global__ void __launch_bounds__(QMAP_TILE) qmap_expand_kernel(QuadricMapParams p)
{
    const int b = blockIdx.x / p.nExpandTiles, j = blockIdx.x - b * p.nExpandTiles;
    int nL, nM;
    if (!qmap_frame(p, b, nL, nM) || p.probOff[b] < 0) return;
    const int nk = p.nLh[b];
    const long long w = (long long)nL + 1, total = (long long)nM * w;
    const double *cp = p.cprobs + p.cprobOff[b];
    const int *rows = p.rowIdx + (long long)b * p.maxKeep;
    double *out = p.probs + p.probOff[b];
    for (long long i = (long long)j * QMAP_TILE + threadIdx.x; i < total; i += (long long)p.nExpandTiles * QMAP_TILE) {
        const long long m = i / w, q = i - m * w;
        double v = 0.0;
        if (nk >= 0) {
            if (q == nL) {
                v = cp[m * (nk + 1) + nk];
            } else {
                int lo = 0, hi = nk;  // first l with rows[l] >= q
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (rows[mid] < q) lo = mid + 1; else hi = mid;
                }
                if (lo < nk && rows[lo] == q) v = cp[m * (nk + 1) + lo];
            }
        }
        out[i] = v;
    }
}

hipError_t launch_quadric_map_gate(const QuadricMapParams &p, hipStream_t stream)
{
    const int tiles = p.B * p.nTiles;
    hipLaunchKernelGGL(qmap_min_kernel, dim3(tiles), dim3(QMAP_TILE), 0, stream, p);
    hipLaunchKernelGGL(qmap_colmin_kernel, dim3(p.B), dim3(QMAP_MAX_COLS), 0, stream, p);
    hipLaunchKernelGGL(qmap_flag_kernel, dim3(tiles), dim3(QMAP_TILE), 0, stream, p);
    hipLaunchKernelGGL(qmap_scan_kernel, dim3(p.B), dim3(QMAP_TILE), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_quadric_map_fill(const QuadricMapParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(qmap_rows_kernel, dim3(p.B * p.nTiles), dim3(QMAP_TILE), 0, stream, p);
    hipLaunchKernelGGL(qmap_fill_kernel, dim3(p.B * p.nKeepTiles), dim3(QMAP_TILE), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_quadric_map_expand(const QuadricMapParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(qmap_expand_kernel, dim3(p.B * p.nExpandTiles), dim3(QMAP_TILE), 0, stream, p);
    return hipGetLastError();
}

#ifdef __HIPCC__
// registers, scratch and LDS of the three kernels that compute costs (tools/bench_quadric_map.py reports them)
hipError_t quadric_map_kernel_usage(int which, int *vgprs, int *scratchBytes, int *ldsBytes)
{
    hipFuncAttributes a;
    const void *f = which == 0 ? reinterpret_cast<const void *>(qmap_min_kernel)
                  : which == 1 ? reinterpret_cast<const void *>(qmap_flag_kernel)
                               : reinterpret_cast<const void *>(qmap_fill_kernel);
    const hipError_t e = hipFuncGetAttributes(&a, f);
    if (e != hipSuccess) return e;
    *vgprs = a.numRegs;
    *scratchBytes = (int)a.localSizeBytes;
    *ldsBytes = (int)a.sharedSizeBytes;
    return hipSuccess;
}
#endif

}  // namespace kb
