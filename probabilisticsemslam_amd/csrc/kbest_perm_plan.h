// kbest_perm_plan.h -- what the two kernels on the column-subset layers must agree on with perm_plan (kbest_perm.hip: the marginals;
// kbest_sample.hip: draws from the joint posterior): the gate, the workgroup size and the LDS plan.
#ifndef KBEST_PERM_PLAN_H
#define KBEST_PERM_PLAN_H

#include <hip/hip_runtime.h>

namespace kb {

constexpr double PM_GATE = 42.0;  // assignment.cpp:9

// threads that accumulate the marginals of a frame of M columns: 4 subsets each, whole waves, at most the largest workgroup.
// (The reduction over the workgroup costs 6 M DPP steps per thread and row whatever the thread has added up before, so fewer,
//  busier threads do less work in all -- but a row is a chain of dependent LDS / L2 reads, and more waves hide it.  Measured in one
//  run, 8 against 4 subsets per thread: profiles/permanent_spt_ab.json, NOTES.md section 13.  The rule is part of the result's
//  bits: the order of the sums follows from it.)
constexpr int PM_SPT = 4;
__host__ __device__ inline int perm_threads(int M)
{
    const int t = (1 << M) / PM_SPT;
    return t < 64 ? 64 : t > 1024 ? 1024 : t;
}

struct PermLds {  // byte offsets into the dynamic LDS
    int red, colMin, waveMin, ctl, rawRow, mask, act, a, g, hist, total;
};

__host__ __device__ inline PermLds perm_lds(int mode, int maxRawRow, int maxCol)
{
    PermLds l;
    int o = 0;
    l.red = o;     o += 2 * 16 * 16 * 8;  // [2][wave][column]
    l.colMin = o;  o += 16 * 8;
    l.waveMin = o; o += 16 * 8;
    l.ctl = o;     o += 16;               // double blockMin; int nKept; int nAct
    const int rows2 = (2 * maxRawRow + 7) & ~7;
    l.rawRow = o;  o += rows2;            // u16: raw row of every kept row
    l.mask = o;    o += rows2;            // u16: non-zero columns of every kept row
    l.act = o;     o += rows2;            // u16: kept index of every active (non-zero) row
    l.a = o;       if (mode < 2) o += maxRawRow * maxCol * 8;
    l.g = o;       if (mode < 2) o += (2 << maxCol) * 8;
    l.hist = o;    if (mode < 1) o += (maxRawRow << maxCol) * 8;
    l.total = (o + 15) & ~15;
    return l;
}

}  // namespace kb
#endif
