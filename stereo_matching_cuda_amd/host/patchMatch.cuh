// patchMatch.cuh -- PatchMatch stereo (Bleyer, Rhemann, Rother, BMVC 2011; not a stage of the reference): a disparity plane per
// pixel, scored over an adaptive-weight window that lies in the plane.  The contract is the comment above smx_pm_params in
// include/smx.h; the twin is its sequential restatement, with its own table and hash (no libsmx_hip.so in it).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// left / right: gray u8 [h][w].  planes [2][3][h][w] = (a, b, d0) of the left and the right view; cost, disp, label [2][h][w].
// GPU result (smx_patchmatch); with host_gpu_compare the twin redoes both views and check_errors compares all four.
void patch_match(unsigned char* left, unsigned char* right, float* planes, float* cost, float* disp, float* label, const int w,
                 const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p, bool host_gpu_compare);
void patchMatchOnCPU(const unsigned char* left, const unsigned char* right, float* planes, float* cost, float* disp, float* label,
                     const int w, const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p);
// the plane costs of given planes of both views, no search (the twin of smx_pm_plane_cost)
void pmPlaneCostOnCPU(const unsigned char* left, const unsigned char* right, const float* planes, float* cost, const int w,
                      const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p);
