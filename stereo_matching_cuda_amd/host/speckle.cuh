// speckle.cuh -- speckle removal on the LR-checked left map (not a stage of the reference: smx_main --speckle).
// Host pointers in / out like the reference-named stage functions; the contract is smx_speckle_filter's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// out = disparity with the pixels of every connected component of at most p.max_size pixels set to new_val (4-neighbours
// that count against vmin and differ by at most p.max_diff).  host_gpu_compare: the CPU twin runs as well and
// check_errors compares.
void speckle_filter(float* disparity, float* out, const int w, const int h, float vmin, float new_val,
                    const smx_speckle_params& p, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp)
void speckle_filterOnCPU(const float* disparity, float* out, const int w, const int h, float vmin, float new_val,
                         const smx_speckle_params& p);
