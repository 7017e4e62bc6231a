// svgf_atrous_lane.hip — the plain a-trous levels on the lane-marching kernel (svgf_atrous_lane_impl.h): steps 1 .. 32.
#include "svgf_atrous_lane_impl.h"

hipError_t launch_atrous_lane(const AtrousArgs &a, hipStream_t s)
{
    if (a.tin || a.tout) return hipErrorInvalidValue;                 // cross-level reuse of the geometric terms: svgf_atrous_lane_reuse.hip (experiments build)
    switch (a.step) {
    case 1: return a.dst ? launch_lane_cfg<0, true>(a, s) : launch_lane_cfg<0, false>(a, s);
    case 2: return a.dst ? launch_lane_cfg<1, true>(a, s) : launch_lane_cfg<1, false>(a, s);
    case 4: return a.dst ? launch_lane_cfg<2, true>(a, s) : launch_lane_cfg<2, false>(a, s);
    case 8: return a.dst ? launch_lane_cfg<3, true>(a, s) : launch_lane_cfg<3, false>(a, s);
    case 16: return a.dst ? launch_lane_cfg<4, true, 3>(a, s) : launch_lane_cfg<4, false, 3>(a, s);
    case 32: return a.dst ? launch_lane_cfg<5, true, 3>(a, s) : launch_lane_cfg<5, false, 3>(a, s);
    default: return hipErrorInvalidValue;
    }
}

#ifdef SVGF_BUILD_EXPERIMENTS
// svgf_exp_atrous_geometry: the workgroup of the plain level of a.step
void atrous_lane_block(const AtrousArgs &a, int *threads, int *lds_bytes)
{
    const int l = atrous_step_log2(a.step);
    *threads = NT;
    *lds_bytes = l == 0 ? LaneLayout<0, 0, 0, 0>::lds_bytes : l == 1 ? LaneLayout<1, 1, 0, 0>::lds_bytes : l == 2 ? LaneLayout<2, 2, 0, 0>::lds_bytes
               : l == 3 ? LaneLayout<3, 3, 0, 0>::lds_bytes : l == 4 ? LaneLayout<4, 3, 0, 0>::lds_bytes : LaneLayout<5, 3, 0, 0>::lds_bytes;
}
#endif
