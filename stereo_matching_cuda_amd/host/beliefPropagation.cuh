// beliefPropagation.cuh -- hierarchical belief propagation on one whole cost volume (not a stage of the reference: smx_main
// --aggregation bp).  Host pointers in / out like sgm_aggregate (sgm.cuh); the contract is smx_bp_aggregate's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// cost: size_d*w*h floats, [z][y][x].  agg (may be NULL): the belief S in the same layout; best: the winner's S; disp_map:
// dmin + z*, z* the last slice of minimal S.  host_gpu_compare: the CPU twin runs as well and check_errors compares.
void belief_propagation(float* cost, float* agg, float* best, float* disp_map, const int w, const int h, const int size_d,
                        const int dmin, const smx_bp_params& p, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp)
void beliefPropagationOnCPU(const float* cost, float* agg, float* best, float* disp_map, const int w, const int h,
                            const int size_d, const int dmin, const smx_bp_params& p);
