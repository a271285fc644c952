// kbest_quadric_map_sample.hip -- the last step of kbest_quadric_map_sample_assoc_batch_f64_dev: the sampler has drawn on a frame's
// COMPACT block (kept landmark rows 0 .. nKeep - 1 in ascending order, then the nM dummy rows), so assign[s][c] is a compact row.
// The kernel here rewrites the caller's d_assign in place into the numbering of the notional raw (nL + nM) x nM block, which is
// what every other sampling entry returns:
//
//   v < 0      stays -1                 (the frame was not drawn)
//   v < nKeep  becomes rowIdx[b][v]     (a kept landmark)
//   otherwise  becomes nL + (v - nKeep) (the miss row of measurement v - nKeep: a miss is not folded into nL)
//
//   qmap_sample_rows_kernel   QMAP_TILE threads a workgroup, workgroup b * nTiles + tile, a grid-stride loop over the frame's
//                             nSample * nM elements: every element read once and written at most once, by one thread
//
// A frame within the launch bounds that keeps more than maxKeep rows was handed to the sampler as nL = -1, which touches nothing of
// it: the kernel writes every assign -1 and every logProb NaN.  A frame beyond the bounds is not touched.  No atomics, no workgroup
// waits for another; every element index is 64-bit.
#include <hip/hip_runtime.h>

#include "kbest_quadric_map.h"

namespace kb {

// A frame the launch takes: qmap_frame of kbest_quadric_map.hip restated -- that one is local to its file and takes the gate
// passes' arguments -- with the offsets of the draws beside it (tests/cpp/quadric_map_sample_host.cpp holds the two against each
// other).  Uniform over a workgroup.
__device__ __forceinline__ bool qmap_sample_frame(const QuadricMapSampleParams &p, int b, int &nL, int &nM)
{
    nL = p.nL[b];
    nM = p.nM[b];
    return nM >= 1 && nM <= p.maxCol && nL >= 0 && nL <= p.maxMap && p.landOff[b] >= 0 && p.measOff[b] >= 0 && p.asgOff[b] >= 0 &&
           p.lpOff[b] >= 0;
}

__global__ void __launch_bounds__(QMAP_TILE) qmap_sample_rows_kernel(QuadricMapSampleParams p)
{
    const int b = blockIdx.x / p.nTiles, j = blockIdx.x - b * p.nTiles;
    int nL, nM;
    if (!qmap_sample_frame(p, b, nL, nM)) return;
    const int nk = p.nKeep[b];  // the TRUE count (qmap_scan_kernel), also beyond maxKeep
    if (nk < 0) return;
    const long long total = (long long)p.nSample * nM, step = (long long)p.nTiles * QMAP_TILE;
    int *asg = p.assign + p.asgOff[b];
    if (nk > p.maxKeep) {  // refused: the sampler saw nL = -1 and wrote nothing
        double *lp = p.logProb + p.lpOff[b];
        for (long long i = (long long)j * QMAP_TILE + threadIdx.x; i < total; i += step) {
            asg[i] = -1;
            if (i < p.nSample) lp[i] = __longlong_as_double(0x7ff8000000000000LL);  // (nM >= 1: total >= nSample)
        }
        return;
    }
    const int *rows = p.rowIdx + (long long)b * p.maxKeep;
    for (long long i = (long long)j * QMAP_TILE + threadIdx.x; i < total; i += step) {
        const int v = asg[i];
        if (v >= 0) asg[i] = v < nk ? rows[v] : nL + (v - nk);  // (v < nk <= maxKeep: inside the frame's rowIdx)
    }
}

hipError_t launch_quadric_map_sample_rows(const QuadricMapSampleParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(qmap_sample_rows_kernel, dim3(p.B * p.nTiles), dim3(QMAP_TILE), 0, stream, p);
    return hipGetLastError();
}

#ifdef __HIPCC__
// registers, scratch and LDS of the kernel (tools/bench_quadric_map_sample.py reports them)
hipError_t quadric_map_sample_kernel_usage(int *vgprs, int *scratchBytes, int *ldsBytes)
{
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void *>(qmap_sample_rows_kernel));
    if (e != hipSuccess) return e;
    *vgprs = a.numRegs;
    *scratchBytes = (int)a.localSizeBytes;
    *ldsBytes = (int)a.sharedSizeBytes;
    return hipSuccess;
}
#endif

}  // namespace kb
