// kbest_wave_sum.h -- the fixed-order fp64 wave sum of the exact tiers (kbest_perm.hip, kbest_cluster.hip, kbest_bigcluster.hip,
// kbest_frontier.hip): part of their results' bits.  Needs dpp_f64, the device's from kbest_wave.h or a host emulation's, before it.
#ifndef KBEST_WAVE_SUM_H
#define KBEST_WAVE_SUM_H

#include "kbest_wave.h"

namespace kb {

// fp64 sum over the 64 lanes in ONE fixed order; valid in lane 63 only.  All lanes must be active.
__device__ __forceinline__ double wave_sum63_f64(double x)
{
    x = x + dpp_f64<0xB1, 0xF>(x);   // quad_perm [1,0,3,2]
    x = x + dpp_f64<0x4E, 0xF>(x);   // quad_perm [2,3,0,1]
    x = x + dpp_f64<0x141, 0xF>(x);  // row_half_mirror
    x = x + dpp_f64<0x140, 0xF>(x);  // row_mirror
    x = x + dpp_f64<0x142, 0xA>(x);  // row_bcast:15 -> rows 1,3
    x = x + dpp_f64<0x143, 0xC>(x);  // row_bcast:31 -> rows 2,3
    return x;
}

}  // namespace kb
#endif
