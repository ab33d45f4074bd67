// crossAggregation.cuh -- cross-based aggregation over one whole cost volume (not a stage of the reference: smx_main
// --aggregation cross).  Host pointers in / out like compute_colour_guided_filter (colourGuidedFilter.cuh); the contract is
// smx_cross_aggregate's (include/smx.h, above smx_cross_workspace_bytes).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// guide: h*w*channels bytes, channels 1 (gray), 3 or 4 (a fourth byte is ignored); cost: size_d*w*h floats, [z][y][x].
// filter_cost / disp_map are IN/OUT like compute_guided_filter's: a pixel is updated iff filter_cost >= min_z q[z]; agg (may be
// NULL): q in the layout of cost.  host_gpu_compare: the CPU twin runs as well and check_errors compares.
void cross_aggregate(unsigned char* guide, int channels, float* cost, float* filter_cost, float* disp_map, float* agg,
                     const int w, const int h, const int size_d, const int dmin, const smx_cross_params& p, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp): scalar, arm by arm and pixel by pixel
void cross_aggregateOnCPU(const unsigned char* guide, int channels, const float* cost, float* filter_cost, float* disp_map,
                          float* agg, const int w, const int h, const int size_d, const int dmin, const smx_cross_params& p);
