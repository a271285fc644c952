// ref_boxes_shim.cpp -- C entry points around VERBATIM SLICES of the reference's stereo box matching.
//
// TEST INFRASTRUCTURE ONLY (see oracle/kbest_oracle.c for the rules).
// This file holds no reference code.  boundBox.h and assignment.cpp as wholes cannot be compiled here (they pull in
// gtsam_quadrics::AlignedBox2, GTSAM, Eigen and OpenCV), but the box code itself is std-only.  oracle/Makefile
// therefore cuts these line ranges out of the reference where it lies --
//     boundBox.h:62-75                  boundBox::IoU, the member function as it stands       (REF_BOXES_IOU_SLICE)
//     constsUtils.h:10                  inf_d                                                 (REF_BOXES_CONSTS_SLICE)
//     assignment.cpp:724-797            asgnBB, computeBBCostMatrix                           (REF_BOXES_ASSIGN_SLICE)
// -- into temporary files under /tmp (never into the repository) and hands their paths to this translation unit.
// What the slices need beyond the std headers is supplied below: a stand-in `boundBox` that holds the five numbers
// the box code reads (the aligned box's corners and xOffset) with the accessors of boundBox.h:21-25, area() being
// width times height as AlignedBox2 has it, and a stand-in `semConsts` with the one setting asgnBB reads.  The IoU
// arithmetic, the asymmetric min of the two IoUs, the -inf fill, the place of the gate, the k = 1 maximise call and
// the epilogue are the reference's own text.  The result, oracle/_ref/libref_boxes.so (git-ignored, a binary), is
// linked against the unmodified reference solver and is used to record tests/golden/boxes_golden.npz and to pin the
// oracle's orc_bb_costs / orc_asgn_bb.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <iostream>
#include <limits>
#include <vector>

#include "shortestPathCPP.hpp"

struct boundBox {
    double x0, y0, x1, y1;  // the aligned box (boundBox.h:13)
    double xOffset;         // boundBox.h:17
    double xmin() const { return x0; }
    double xmax() const { return x1; }
    double ymin() const { return y0; }
    double ymax() const { return y1; }
    double area() const { return (x1 - x0) * (y1 - y0); }  // width() * height()
#include REF_BOXES_IOU_SLICE
};

struct semConsts {
    double NONASSIGN_BOUNDBOX;
};

std::vector<double> computeBBCostMatrix(const std::vector<boundBox> &bbL, const std::vector<boundBox> &bbR, const semConsts &runConsts);

#include REF_BOXES_CONSTS_SLICE
#include REF_BOXES_ASSIGN_SLICE

static std::vector<boundBox> boxes(const double *b, int n)
{
    std::vector<boundBox> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = boundBox{b[5 * i], b[5 * i + 1], b[5 * i + 2], b[5 * i + 3], b[5 * i + 4]};
    return v;
}

extern "C" {

// computeBBCostMatrix (assignment.h, assignment.cpp:777-797).  Boxes are (xmin, ymin, xmax, ymax, xOffset);
// out: (nR + nL) x nL column-major.
void ref_bb_costs(const double *L, int nL, const double *R, int nR, double gate, double *out)
{
    const semConsts c{gate};
    const std::vector<double> m = computeBBCostMatrix(boxes(L, nL), boxes(R, nR), c);
    std::copy(m.begin(), m.end(), out);
}

// asgnBB (assignment.h:21, assignment.cpp:724-775).  asg[nL]: the right box of every left box, or -1.
void ref_asgn_bb(const double *L, int nL, const double *R, int nR, double gate, int32_t *asg)
{
    const semConsts c{gate};
    const std::vector<int> a = asgnBB(boxes(L, nL), boxes(R, nR), c);
    for (size_t i = 0; i < a.size(); i++) asg[i] = a[i];
}

}  // extern "C"
