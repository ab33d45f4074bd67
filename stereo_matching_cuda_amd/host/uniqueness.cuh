// uniqueness.cuh -- the uniqueness (peak-ratio) test on the LR-checked left map (not a stage of the reference: smx_main
// --uniqueness).  The contract is smx_dev_uniqueness's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// CPU twin (cpu_twins.cpp), from the aggregated volume agg [size_d][h][w] of the view the map belongs to: the winner by the
// key's rule, sec BY THE DEFINITION -- the smallest cost over the slices at least two away from the final winner, found by a
// loop over all of them, not by the streaming form of the kernels --, then the test.  out = disparity with the rejected
// pixels that count against vmin set to new_val; margin (may be nullptr) = sec - c0, +inf where sec is unknown, NaN where
// the pixel has no winner.
void uniqueness_onCPU(const float* agg, const float* disparity, float* out, float* margin, const int w, const int h,
                      const int size_d, float ratio, float vmin, float new_val);
