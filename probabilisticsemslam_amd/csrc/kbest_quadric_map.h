// kbest_quadric_map.h -- arguments and launchers of kbest_quadric_map.hip, for that file and the C API.
#ifndef KBEST_QUADRIC_MAP_H
#define KBEST_QUADRIC_MAP_H

#include "kbest_engine.h"

namespace kb {

// kbest_quadric_map.hip: a frame's conditioned compact block from quadrics against a large map (kbest_c.h, "Exact
// getAssignmentProbs from quadrics").  Grids are one-dimensional: workgroup b * nTiles + tile of the passes over the landmark rows.
constexpr int QMAP_TILE = 256;      // landmark rows (threads) per workgroup of the gate passes: KBEST_QUADRIC_MAP_TILE
constexpr int QMAP_MAX_COLS = 128;  // measurements per frame at the most
struct QuadricMapParams {
    const double *mapMean, *mapCov;     // the call's map: [nMap][3], [nMap][9]
    const double *measMean, *measCov;   // measurements of all frames
    const long long *landOff, *measOff; // [B] frame b sees landmarks landOff[b] .. + nL[b] of the map, has measurements from measOff[b]
    const int *nL, *nM;                 // [B]
    double gate;
    int B, maxMap, maxKeep, maxCol;
    int nTiles;                         // ceil(maxMap / QMAP_TILE), at least 1: tiles per frame of the launch
    int nKeepTiles;                     // ceil(maxKeep / QMAP_TILE), at least 1: workgroups per frame of the fill
    int nExpandTiles;                   // workgroups per frame of the expansion
    double *tileMin;                    // [B][nTiles][maxCol]
    double *colMin;                     // [B][maxCol]
    u64 *keep;                          // [B][nTiles][QMAP_TILE / 64] ballots of the kept rows
    int *tileCnt, *tileOff;             // [B][nTiles]
    int *nKeep;                         // [B] out: kept landmark rows, the true count
    int *nLh;                           // [B] nKeep, or -1 where the frame is not taken or keeps more than maxKeep rows
    long long *costOff, *cprobOff;      // [B] b (maxKeep + maxCol) maxCol and b maxCol (maxKeep + 1)
    int *rowIdx;                        // [B][maxKeep] out
    double *ccost;                      // the compact blocks
    const double *cprobs;               // expansion: the compact probabilities, the dense ones and their offsets
    double *probs;
    const long long *probOff;
};
hipError_t launch_quadric_map_gate(const QuadricMapParams &p, hipStream_t stream);    // tileMin, colMin, keep, tileCnt, tileOff, nKeep, nLh
hipError_t launch_quadric_map_fill(const QuadricMapParams &p, hipStream_t stream);    // rowIdx, ccost
hipError_t launch_quadric_map_expand(const QuadricMapParams &p, hipStream_t stream);  // probs
hipError_t quadric_map_kernel_usage(int which, int *vgprs, int *scratchBytes, int *ldsBytes);

// kbest_quadric_map_sample.hip: the draws of the sampler on the compact blocks, rewritten in place from compact rows to the rows of
// the notional raw (nL + nM) x nM block (kbest_c.h, "Joint associations from quadrics").  Workgroup b * nTiles + tile.
struct QuadricMapSampleParams {
    const long long *landOff, *measOff; // [B] as QuadricMapParams': with nL and nM they say whether the launch takes the frame
    const int *nL, *nM;                 // [B]
    int B, maxMap, maxKeep, maxCol;
    int nTiles;                         // workgroups per frame: a grid-stride loop over the frame's nSample * nM elements
    int nSample;
    const int *nKeep;                   // [B] the true count of kept rows; beyond maxKeep: -1s and NaNs
    const int *rowIdx;                  // [B][maxKeep]
    int *assign;                        // in and out: frame b's [nSample][nM] at asgOff[b]
    const long long *asgOff;
    double *logProb;                    // frame b's [nSample] at lpOff[b]: written only where nKeep > maxKeep
    const long long *lpOff;
};
hipError_t launch_quadric_map_sample_rows(const QuadricMapSampleParams &p, hipStream_t stream);
hipError_t quadric_map_sample_kernel_usage(int *vgprs, int *scratchBytes, int *ldsBytes);

}  // namespace kb
#endif
