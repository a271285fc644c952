// kbest_costs.hip -- cost-matrix construction on the device: the producers of the
// k-best path's input, so that a frame's association runs on the GPU from (means, covariances) or bounding boxes
// to probabilities / matches without the cost matrix ever visiting the host.
#include <hip/hip_runtime.h>

#include "kbest_engine.h"
#include "kbest_quadric.h"

namespace kb {

__device__ __forceinline__ double c_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// computeQuadricCostMatrix (assignment.cpp:705-722): one workgroup per frame, one thread per (landmark,
// measurement) pair; +inf everywhere else except the gate value on each column's own dummy row (:713-720).
__global__ void __launch_bounds__(256) quadric_cost_kernel(QuadricParams p)
{
    const int b = blockIdx.x;
    const int nL = p.nL[b], nM = p.nM[b], nR = nL + nM;
    const double *m1 = p.landMean + 3 * p.landOff[b], *c1 = p.landCov + 9 * p.landOff[b];
    const double *m2 = p.measMean + 3 * p.measOff[b], *c2 = p.measCov + 9 * p.measOff[b];
    double *out = p.cost + p.costOff[b];
    for (int i = threadIdx.x; i < nR * nM; i += blockDim.x) {
        const int c = i / nR, r = i - c * nR;
        double val = c_inf();
        if (r < nL) {
            double d[3], S[9], x[3];
#pragma unroll
            for (int j = 0; j < 3; j++) d[j] = m1[r * 3 + j] - m2[c * 3 + j];
#pragma unroll
            for (int j = 0; j < 9; j++) S[j] = c1[r * 9 + j] + c2[c * 9 + j];
            ldlt3_solve(S, d, x);
            val = d[0] * x[0] + d[1] * x[1] + d[2] * x[2];
        } else if (r == nL + c) {
            val = p.gate;
        }
        out[i] = val;
    }
}

// boundBox::IoU (boundBox.h:62-75): `a` is *this (its xOffset is applied), `o` is the other box.
__device__ __forceinline__ double bb_iou(const double *a, const double *o)
{
    const double l = fmax(a[0] + a[4], o[0]), r = fmin(a[2] + a[4], o[2]);
    const double t = fmax(a[1], o[1]), bt = fmin(a[3], o[3]);
    if (l >= r || t >= bt) return 0.0;
    const double inter = (r - l) * (bt - t);
    const double areaA = (a[2] - a[0]) * (a[3] - a[1]), areaO = (o[2] - o[0]) * (o[3] - o[1]);
    return inter / (areaA + areaO - inter);
}

// computeBBCostMatrix (assignment.cpp:777-797): rows = right boxes + one dummy per left box, columns = left boxes,
// profits = min of the two (asymmetric) IoUs, -inf fill, gate profit on the dummies.
__global__ void __launch_bounds__(256) bb_cost_kernel(BoxParams p)
{
    const int b = blockIdx.x;
    const int nL = p.nL[b], nR = p.nR[b], nRows = nR + nL;
    const double *L = p.boxL + 5 * p.offL[b], *R = p.boxR + 5 * p.offR[b];
    double *out = p.cost + p.costOff[b];
    for (int i = threadIdx.x; i < nRows * nL; i += blockDim.x) {
        const int c = i / nRows, r = i - c * nRows;
        double val = -c_inf();
        if (r < nR) {
            const double i1 = bb_iou(R + 5 * r, L + 5 * c), i2 = bb_iou(L + 5 * c, R + 5 * r);
            val = i1 < i2 ? i1 : i2;
        } else if (r == nR + c) {
            val = p.gate;
        }
        out[i] = val;
    }
}

// asgnBB epilogue (assignment.cpp:769-773): column c matched to right box row4col[c] unless that is a dummy.
__global__ void __launch_bounds__(64) bb_assign_kernel(BoxParams p, const int *row4col, const int *nf, int k, int maxCol)
{
    const int b = blockIdx.x;
    const int nL = p.nL[b], nR = p.nR[b];
    for (int c = threadIdx.x; c < nL; c += 64) {
        int a = -1;
        if (nf[b] > 0) { const int r = row4col[(long long)b * k * maxCol + c]; if (r < nR) a = r; }
        p.assign[p.offL[b] + c] = a;
    }
}

hipError_t launch_quadric_costs(const QuadricParams &p, int B, hipStream_t stream)
{
    hipLaunchKernelGGL(quadric_cost_kernel, dim3(B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_bb_costs(const BoxParams &p, int B, hipStream_t stream)
{
    hipLaunchKernelGGL(bb_cost_kernel, dim3(B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_bb_assign(const BoxParams &p, const int *row4col, const int *nf, int k, int maxCol, int B,
                            hipStream_t stream)
{
    hipLaunchKernelGGL(bb_assign_kernel, dim3(B), dim3(64), 0, stream, p, row4col, nf, k, maxCol);
    return hipGetLastError();
}


// toProbs (assignment.h:19, assignment.cpp:527-542): m = std::min_element of the vector; x -> exp(m - x) where m + 42 > x, else 0.
// One workgroup; in place.  (The reference uses it on the permanent path only; it is elementwise, so this is all of it.)
__global__ void __launch_bounds__(256) to_probs_kernel(double *x, long long n)
{
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const double x0 = n > 0 ? x[0] : 0.0;  // (read before the barriers below: the second loop overwrites it)
    double m = c_inf();
    for (long long i = tid; i < n; i += 256) m = x[i] < m ? x[i] : m;  // std::min_element: first minimum, same value
    red[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] = red[tid + w] < red[tid] ? red[tid + w] : red[tid];
        __syncthreads();
    }
    // std::min_element starts from the FIRST element and moves on only where another compares less: a NaN there stays the
    // "minimum" (nothing compares less than it), and every output is 0.  A NaN anywhere else never compares less and is skipped.
    m = x0 != x0 ? x0 : red[0];
    const double GATE = 42.0;  // assignment.cpp:9
    for (long long i = tid; i < n; i += 256) {
        const double c = x[i];
        x[i] = (m + GATE > c) ? exp(m - c) : 0.0;  // :536-540
    }
}

hipError_t launch_to_probs(double *x, long long n, hipStream_t stream)
{
    hipLaunchKernelGGL(to_probs_kernel, dim3(1), dim3(256), 0, stream, x, n);
    return hipGetLastError();
}

}  // namespace kb
