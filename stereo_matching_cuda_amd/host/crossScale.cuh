// crossScale.cuh -- cross-scale cost aggregation (Zhang et al., CVPR 2014; not a stage of the reference): the CPU twins of the
// pyramid and of the combination with its winners.  The contract is smx_pyr_down's and smx_cscale_combine's (include/smx.h,
// above smx_cscale_params); the level geometry and the weights are those of smx_cscale_level and smx_cscale_weights
// (csrc/smx_cscale_host.h, the code the library runs).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// src [h][w][channels] u8 (channels 1, 3 or 4) -> dst [(h+1)/2][(w+1)/2][channels]
void pyrDownOnCPU(const unsigned char* src, unsigned char* dst, const int w, const int h, const int channels);
// levels: p.scales volumes of one view, level s [size_d_s][h_s][w_s]; out: the combined volume [size_d][h][w]; best / disp_map:
// the winners' costs (-0 as +0) and labels dmin + slice, h*w floats each, either may be NULL.  A pixel without a winner (every
// cost a NaN) gets what smx_cscale_combine unpacks from the identity key: the NaN 0x7FFFFFFF and the label dmin.
void crossScaleOnCPU(const float* const* levels, float* out, float* best, float* disp_map, const int w, const int h, const int dmin,
                     const int size_d, const smx_cscale_params& p);
