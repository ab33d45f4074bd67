// regionVoting.cuh -- region voting and 16-direction interpolation on the cross arms of the left guide (not a stage of the
// reference: smx_main --vote).  Host pointers in / out like speckle_filter (speckle.cuh); the contract is smx_region_vote's
// (include/smx.h, above smx_vote_workspace_bytes).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// guide: h*w*channels bytes, channels 1 (gray), 3 or 4 (a fourth byte is ignored); disparity: the left map behind the LR check,
// uniqueness and speckle stages; disparity_right: the right winner-take-all map (may be NULL: every remaining outlier is an
// occlusion then); out: the voted map.  arms: l1, l2, tau1, tau2 of the support regions.  host_gpu_compare: the CPU twin runs as
// well and check_errors compares.
void region_vote(unsigned char* guide, int channels, float* disparity, float* disparity_right, float* out, const int w,
                 const int h, const int dmin, const int size_d, const smx_vote_params& p, const smx_cross_params& arms,
                 bool host_gpu_compare);
// CPU twin (cpu_twins.cpp): scalar, pixel by pixel; d_lr is smx_config().params.d_lr, like detect_occlusionOnCPU's
void region_voteOnCPU(const unsigned char* guide, int channels, const float* disparity, const float* disparity_right, float* out,
                      const int w, const int h, const int dmin, const int size_d, const smx_vote_params& p,
                      const smx_cross_params& arms);
