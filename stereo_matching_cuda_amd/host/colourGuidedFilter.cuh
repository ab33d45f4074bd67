// colourGuidedFilter.cuh -- the guided filter with a colour (RGB) guide over one whole cost volume (not a stage of the
// reference: smx_main --guidance rgb).  Host pointers in / out like compute_guided_filter (guidedFilter.cuh); the contract is
// smx_colour_guided_filter's (include/smx.h, above smx_cgf_workspace_bytes).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// rgb: h*w*channels bytes, channels 3 or 4 (R, G, B first); cost: size_d*w*h floats, [z][y][x].  filter_cost / disp_map are
// IN/OUT like compute_guided_filter's: a pixel is updated iff filter_cost >= min_z q[z]; agg (may be NULL): q in the layout of
// cost.  radius and eps come from smx_config().params.  host_gpu_compare: the CPU twin runs as well and check_errors compares.
void compute_colour_guided_filter(unsigned char* rgb, int channels, float* cost, float* filter_cost, float* disp_map, float* agg,
                                  const int w, const int h, const int size_d, const int dmin, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp); radius and eps explicit
void colour_guided_filterOnCPU(const unsigned char* rgb, int channels, const float* cost, float* filter_cost, float* disp_map,
                               float* agg, const int w, const int h, const int size_d, const int dmin, const int radius,
                               const double eps);
