// wmf.cuh -- the weighted-median refinement of the filled left map (not a stage of the reference: smx_main --wmf).
// Host pointers in / out like the reference-named stage functions; the contract is smx_weighted_median's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// out = weighted median of disparity guided by `guide`, labels [dmin, dmin + size_d); select == nullptr filters every
// pixel, else the pixels with (int)select < dmin.  host_gpu_compare: the CPU twin runs as well and check_errors compares.
void weighted_median(unsigned char* guide, float* disparity, float* select, float* out, const int w, const int h,
                     int dmin, int size_d, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp)
void weighted_medianOnCPU(const unsigned char* guide, const float* disparity, const float* select, float* out,
                          const int w, const int h, int dmin, int size_d, const smx_wmf_params& p);
