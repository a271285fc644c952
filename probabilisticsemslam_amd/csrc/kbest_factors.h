// kbest_factors.h -- arguments and launcher of kbest_factors.hip, for that file and the C API.
#ifndef KBEST_FACTORS_H
#define KBEST_FACTORS_H

#include <hip/hip_runtime.h>

namespace kb {

// kbest_factors.hip: factor lists from association probabilities (kbest_c.h, "Factor lists from association probabilities").
// Grids are one-dimensional: workgroup b * maxCol + m of the passes over the rows, workgroup b of the scan inside a frame.
constexpr int FACTOR_TILE = 256;      // slots (threads) per chunk of a row
constexpr int FACTOR_MAX_COLS = 128;  // measurements per frame at the most: the threads of the scan inside a frame
struct FactorParams {
    const double *probs;                // frame b's [nM][nSlot + 1] at probOff[b]
    const long long *probOff;           // [B]
    const int *nSlot, *nM;              // [B]
    const int *rowIdx;                  // NULL (dense: slot l is landmark l) or [B][rowStride]
    long long rowStride;
    const long long *landOff;           // NULL (0) or [B]: the map index of a landmark is landOff[b] + landmark
    const int *method;                  // NULL or [B]: a frame with method < 0 emits nothing
    double factorThresh, newThresh, boxSd;
    int B, maxSlot, maxCol;
    long long maxFactor, maxNew;        // capacities of the lists
    int *fFrame, *fMeas, *fLand;        // the factor list
    long long *fMap;                    // may be NULL
    double *fProb, *fSigma;
    int *nFrame, *nMeas;                // the new-landmark list
    double *nProb, *nSigma;
    int *nFactor, *nNew;                // [B] true counts
    long long *factorOff, *newOff;      // [B] exclusive prefix sums of the true counts
    long long *total;                   // [2] the true totals: factors, new landmarks
    int *support;                       // NULL or [nSupport]
    long long nSupport;
    int *rowCnt, *rowNew;               // work space [B][maxCol]: factors of row (b, m) and its new-landmark flag, then (after the
                                        // scan inside the frame) the positions of the row's first entries inside the frame's lists
};
// zero of the support, count, scan inside every frame, scan over the frames, emit: five launches at the most, stream order between
// them.  B = 0: the totals 0 and the support zeroed.
hipError_t launch_assoc_factors(const FactorParams &p, hipStream_t stream);
hipError_t factors_kernel_usage(int which, int *vgprs, int *scratchBytes, int *ldsBytes);  // 0: count, 1: frame scan, 2: batch scan, 3: emit

}  // namespace kb
#endif
