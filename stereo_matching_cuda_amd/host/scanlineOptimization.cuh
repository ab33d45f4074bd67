// scanlineOptimization.cuh -- the scan-line optimiser with colour-adaptive penalties over one whole cost volume (not a stage of
// the reference: smx_main --aggregation scanline / cross-scanline).  Host pointers in / out like sgm_aggregate (sgm.cuh); the
// contract is smx_scanline_optimize's (include/smx.h, above smx_scanline_workspace_bytes).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// guide_own / guide_other: h*w*channels bytes each, channels 1 (gray), 3 or 4 (a fourth byte is ignored): the guide of the
// volume's view and of the other view, where the partner (x + dmin + z, y) of a label lies.  cost: size_d*w*h floats, [z][y][x].
// agg (may be NULL): S in the same layout; best: the winner's S; disp_map: dmin + z*, z* the last slice of minimal S.
// host_gpu_compare: the CPU twin runs as well and check_errors compares.
void scanline_optimize(unsigned char* guide_own, unsigned char* guide_other, int channels, float* cost, float* agg, float* best,
                       float* disp_map, const int w, const int h, const int size_d, const int dmin, const smx_scanline_params& p,
                       bool host_gpu_compare);
// CPU twin (cpu_twins.cpp): scalar, pixel by pixel and label by label
void scanline_optimizeOnCPU(const unsigned char* guide_own, const unsigned char* guide_other, int channels, const float* cost,
                            float* agg, float* best, float* disp_map, const int w, const int h, const int size_d, const int dmin,
                            const smx_scanline_params& p);
