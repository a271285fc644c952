// kbest_factors.hip -- factor lists from association probabilities, on the stream: what the reference's consumer loop
// (system.cpp:279-346) makes of a frame's probabilities, as a stream compaction.
//
//   for m, for q < nL:  if (probs[m][q] < NEW_FACTOR_PROB_THRESH) continue;  two factors with noise BOX_SD / probs[m][q]
//   for m:              if (probs[m][nL] > NEW_LANDMARK_THRESH)              a new landmark, noise BOX_SD / probs[m][nL]
//
// Frame b's probabilities are row-major [nM][nSlot + 1] at probOff[b]; slot nSlot is the miss column, slot l < nSlot the landmark
// rowIdx[b * rowStride + l] (compact form) or l (dense form).  The position of every entry is COMPUTED, never claimed: factor
// (b, m, l) stands at factorOff[b] + (factors of rows < m of the frame) + (kept slots < l of the row), so the lists are in the
// order b, m, l and a frame's entries are the same alone and in any batch.
//
//   factors_zero_kernel         the support counts, a grid-stride loop
//   factors_count_kernel        workgroup b * maxCol + m: the row's factors (ballot, popcount, four wave sums through LDS) and its
//                               new-landmark flag into the work space; 0 for every row that emits nothing
//   factors_frame_scan_kernel   workgroup b, FACTOR_MAX_COLS threads: the exclusive prefix of the frame's rows in place, nFactor, nNew
//   factors_batch_scan_kernel   ONE workgroup: the exclusive prefix over the frames in chunks of FACTOR_TILE with a running base,
//                               factorOff, newOff, total
//   factors_emit_kernel         workgroup b * maxCol + m: the predicates again, the row in chunks of FACTOR_TILE with a running base;
//                               rank inside a wave from ballot and mbcnt, wave bases through LDS; one integer atomicAdd per factor
//                               into the support, whose value does not depend on the order
//
// Stream order is the only synchronisation between the launches.  No floating-point atomics, no grid barrier, no workgroup waits
// for another; every index into a buffer is 64-bit.  A frame emits nothing where method[b] < 0 or it lies outside the bounds
// (factors_frame): its slice may never have been written, and a NaN passes !(p < t).
#include <hip/hip_runtime.h>

#include "kbest_factors.h"

namespace kb {

typedef unsigned long long fu64;

// A frame that emits: uniform over a workgroup.
__device__ __forceinline__ bool factors_frame(const FactorParams &p, int b, int &nSlot, int &nM)
{
    nSlot = p.nSlot[b];
    nM = p.nM[b];
    if (p.method && p.method[b] < 0) return false;
    if (p.landOff && p.landOff[b] < 0) return false;
    return nM >= 1 && nM <= p.maxCol && nSlot >= 0 && nSlot <= p.maxSlot && p.probOff[b] >= 0;
}

__device__ __forceinline__ int factors_lane_rank(fu64 mask)  // set bits of mask below this lane
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

__global__ void __launch_bounds__(FACTOR_TILE) factors_zero_kernel(int *x, long long n)
{
    const long long step = (long long)gridDim.x * FACTOR_TILE;
    for (long long i = (long long)blockIdx.x * FACTOR_TILE + threadIdx.x; i < n; i += step) x[i] = 0;
}

__global__ void __launch_bounds__(FACTOR_TILE) factors_count_kernel(FactorParams p)
{
    __shared__ int sCnt[FACTOR_TILE / 64];
    const int b = blockIdx.x / p.maxCol, m = blockIdx.x - b * p.maxCol, tid = threadIdx.x;
    const long long at = (long long)b * p.maxCol + m;
    int nSlot, nM;
    if (!factors_frame(p, b, nSlot, nM) || m >= nM) {  // (uniform over the workgroup)
        if (tid == 0) {
            p.rowCnt[at] = 0;
            p.rowNew[at] = 0;
        }
        return;
    }
    const double *row = p.probs + p.probOff[b] + (long long)m * ((long long)nSlot + 1);
    int cnt = 0;  // wave-uniform: the kept slots this wave has seen
    for (int l0 = 0; l0 < nSlot; l0 += FACTOR_TILE) {
        const int l = l0 + tid;
        const bool keep = l < nSlot && !(row[l] < p.factorThresh);
        cnt += __popcll(__ballot(keep));
    }
    if ((tid & 63) == 0) sCnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < FACTOR_TILE / 64; w++) sum += sCnt[w];
        p.rowCnt[at] = sum;
        p.rowNew[at] = row[nSlot] > p.newThresh ? 1 : 0;
    }
}

// In place: rowCnt[b][m] and rowNew[b][m] become the exclusive prefixes over the frame's rows (rows m >= nM hold 0).
__global__ void __launch_bounds__(FACTOR_MAX_COLS) factors_frame_scan_kernel(FactorParams p)
{
    __shared__ int sF[2][FACTOR_MAX_COLS], sN[2][FACTOR_MAX_COLS];
    const int b = blockIdx.x, m = threadIdx.x;
    const long long at = (long long)b * p.maxCol + m;
    const int f = m < p.maxCol ? p.rowCnt[at] : 0, n = m < p.maxCol ? p.rowNew[at] : 0;
    sF[0][m] = f;
    sN[0][m] = n;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < FACTOR_MAX_COLS; d <<= 1) {  // Hillis-Steele, inclusive; a frame has fewer than 2^31 factors (128 x 2^22)
        sF[cur ^ 1][m] = sF[cur][m] + (m >= d ? sF[cur][m - d] : 0);
        sN[cur ^ 1][m] = sN[cur][m] + (m >= d ? sN[cur][m - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (m < p.maxCol) {
        p.rowCnt[at] = sF[cur][m] - f;
        p.rowNew[at] = sN[cur][m] - n;
    }
    if (m == FACTOR_MAX_COLS - 1) {
        p.nFactor[b] = sF[cur][m];
        p.nNew[b] = sN[cur][m];
    }
}

__global__ void __launch_bounds__(FACTOR_TILE) factors_batch_scan_kernel(FactorParams p)
{
    __shared__ long long sF[2][FACTOR_TILE], sN[2][FACTOR_TILE];
    const int tid = threadIdx.x;
    long long baseF = 0, baseN = 0;  // uniform: the totals of the chunks before
    for (long long b0 = 0; b0 < p.B; b0 += FACTOR_TILE) {
        const long long b = b0 + tid;
        const long long f = b < p.B ? p.nFactor[b] : 0, n = b < p.B ? p.nNew[b] : 0;
        __syncthreads();  // (the chunk before has read its totals)
        sF[0][tid] = f;
        sN[0][tid] = n;
        __syncthreads();
        int cur = 0;
        for (int d = 1; d < FACTOR_TILE; d <<= 1) {
            sF[cur ^ 1][tid] = sF[cur][tid] + (tid >= d ? sF[cur][tid - d] : 0);
            sN[cur ^ 1][tid] = sN[cur][tid] + (tid >= d ? sN[cur][tid - d] : 0);
            cur ^= 1;
            __syncthreads();
        }
        if (b < p.B) {
            p.factorOff[b] = baseF + sF[cur][tid] - f;
            p.newOff[b] = baseN + sN[cur][tid] - n;
        }
        baseF += sF[cur][FACTOR_TILE - 1];
        baseN += sN[cur][FACTOR_TILE - 1];
    }
    if (tid == 0) {
        p.total[0] = baseF;
        p.total[1] = baseN;
    }
}

__global__ void __launch_bounds__(FACTOR_TILE) factors_emit_kernel(FactorParams p)
{
    __shared__ int sCnt[2][FACTOR_TILE / 64];
    const int b = blockIdx.x / p.maxCol, m = blockIdx.x - b * p.maxCol, tid = threadIdx.x, wave = tid >> 6;
    int nSlot, nM;
    if (!factors_frame(p, b, nSlot, nM) || m >= nM) return;  // (uniform over the workgroup)
    const long long at = (long long)b * p.maxCol + m;
    const double *row = p.probs + p.probOff[b] + (long long)m * ((long long)nSlot + 1);
    const int *rows = p.rowIdx ? p.rowIdx + (long long)b * p.rowStride : nullptr;
    const long long land0 = p.landOff ? p.landOff[b] : 0;
    if (tid == 0) {
        const double q = row[nSlot];
        const long long pos = p.newOff[b] + p.rowNew[at];
        if (q > p.newThresh && pos < p.maxNew) {
            p.nFrame[pos] = b;
            p.nMeas[pos] = m;
            p.nProb[pos] = q;
            p.nSigma[pos] = p.boxSd / q;
        }
    }
    long long base = p.factorOff[b] + p.rowCnt[at];  // uniform: the position of the chunk's first entry
    int turn = 0;
    for (int l0 = 0; l0 < nSlot; l0 += FACTOR_TILE, turn ^= 1) {
        const int l = l0 + tid;
        const double q = l < nSlot ? row[l] : 0.0;
        const bool keep = l < nSlot && !(q < p.factorThresh);
        const fu64 mask = __ballot(keep);
        if ((tid & 63) == 0) sCnt[turn][wave] = __popcll(mask);
        // one barrier a chunk: a wave writes sCnt[turn] again two chunks on, behind the barrier of the chunk between, which every
        // wave reaches only after its reads here
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < FACTOR_TILE / 64; w++) {
            const int c = sCnt[turn][w];
            before += w < wave ? c : 0;
            all += c;
        }
        if (keep) {
            const int land = rows ? rows[l] : l;
            const long long pos = base + before + factors_lane_rank(mask), map = land0 + land;
            if (pos < p.maxFactor) {
                p.fFrame[pos] = b;
                p.fMeas[pos] = m;
                p.fLand[pos] = land;
                if (p.fMap) p.fMap[pos] = map;
                p.fProb[pos] = q;
                p.fSigma[pos] = p.boxSd / q;
            }
            if (p.support && map >= 0 && map < p.nSupport) atomicAdd(p.support + map, 1);
        }
        base += all;
    }
}

hipError_t launch_assoc_factors(const FactorParams &p, hipStream_t stream)
{
    if (p.support && p.nSupport > 0) {
        long long g = (p.nSupport + FACTOR_TILE - 1) / FACTOR_TILE;
        if (g > 1024) g = 1024;
        hipLaunchKernelGGL(factors_zero_kernel, dim3((int)g), dim3(FACTOR_TILE), 0, stream, p.support, p.nSupport);
    }
    if (p.B > 0) {
        hipLaunchKernelGGL(factors_count_kernel, dim3(p.B * p.maxCol), dim3(FACTOR_TILE), 0, stream, p);
        hipLaunchKernelGGL(factors_frame_scan_kernel, dim3(p.B), dim3(FACTOR_MAX_COLS), 0, stream, p);
    }
    hipLaunchKernelGGL(factors_batch_scan_kernel, dim3(1), dim3(FACTOR_TILE), 0, stream, p);
    if (p.B > 0) hipLaunchKernelGGL(factors_emit_kernel, dim3(p.B * p.maxCol), dim3(FACTOR_TILE), 0, stream, p);
    return hipGetLastError();
}

#ifdef __HIPCC__
// registers, scratch and LDS of the passes (tools/bench_factors.py reports them)
hipError_t factors_kernel_usage(int which, int *vgprs, int *scratchBytes, int *ldsBytes)
{
    const void *k = which == 0   ? reinterpret_cast<const void *>(factors_count_kernel)
                    : which == 1 ? reinterpret_cast<const void *>(factors_frame_scan_kernel)
                    : which == 2 ? reinterpret_cast<const void *>(factors_batch_scan_kernel)
                                 : reinterpret_cast<const void *>(factors_emit_kernel);
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, k);
    if (e != hipSuccess) return e;
    *vgprs = a.numRegs;
    *scratchBytes = (int)a.localSizeBytes;
    *ldsBytes = (int)a.sharedSizeBytes;
    return hipSuccess;
}
#endif

}  // namespace kb
