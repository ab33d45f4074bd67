// permeability.cuh -- the information permeability filter (Cigla & Alatan 2013; not a stage of the reference): full-image
// edge-aware aggregation of an f32 volume by four one-dimensional recurrences per slice.  The contract is the comment above
// smx_perm_params in include/smx.h; the twin is its scalar restatement, with the weight table of smx_perm_table
// (csrc/smx_perm_host.h, the code the library runs).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// volume [size_d][h][w] f32, guide u8 [h][w][channels] (channels 1, 3 or 4) -> out [size_d][h][w] (weighted sums, not means);
// best / disp_map: the winners' costs (-0 as +0) and labels dmin + slice, h*w floats each; any output may be NULL.
// GPU result (smx_permeability_filter); with host_gpu_compare the twin redoes it and check_errors compares.
void permeability_filter(float* volume, unsigned char* guide, int channels, float* out, float* best, float* disp_map, const int w,
                         const int h, const int dmin, const int size_d, const smx_perm_params& p, bool host_gpu_compare);
// A pixel without a winner (every cost a NaN) gets what smx_permeability_filter unpacks from the identity key: the NaN
// 0x7FFFFFFF and the label dmin.  out may be NULL.
void permeabilityOnCPU(const float* volume, const unsigned char* guide, const int channels, float* out, float* best, float* disp_map,
                       const int w, const int h, const int dmin, const int size_d, const smx_perm_params& p);
