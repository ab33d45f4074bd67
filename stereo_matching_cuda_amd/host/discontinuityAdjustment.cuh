// discontinuityAdjustment.cuh -- depth-discontinuity adjustment of a label map from its view's aggregated volume (not a stage of
// the reference: smx_main --adjust).  Host pointers in / out like region_vote (regionVoting.cuh); the contract is
// smx_discontinuity_adjust's (include/smx.h, above smx_adjust_workspace_bytes).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// disparity: h*w labels of one view; agg: that view's aggregated volume [size_d][h][w]; out: the adjusted map.  sub: NULL, or h*w
// floats IN/OUT with subpix_mode SMX_SUBPIX_PARABOLA / SMX_SUBPIX_EQUIANGULAR: the pixels whose label changes get their own fit.
// host_gpu_compare: the CPU twin runs as well and check_errors compares.
void discontinuity_adjust(float* disparity, float* agg, float* out, const int w, const int h, const int dmin, const int size_d,
                          const smx_adjust_params& p, int subpix_mode, float* sub, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp): scalar, pixel by pixel
void discontinuityAdjustOnCPU(const float* disparity, const float* agg, float* out, const int w, const int h, const int dmin,
                              const int size_d, const smx_adjust_params& p, int subpix_mode, float* sub);
