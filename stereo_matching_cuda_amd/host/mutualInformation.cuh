// mutualInformation.cuh -- the mutual-information matching cost (not a stage of the reference: smx_main --cost mi).  Host
// pointers in / out like compute_cost (costVolume.cuh); the contracts are smx_mi_histogram's and smx_mi_cost's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// hist: u32 [256][256], the joint histogram of the pixels that the left map `disp` (f32 [h][w], occlusion mark `mark`) pairs up.
// host_gpu_compare: the CPU twin runs as well and the counters are compared.
void compute_mi_histogram(unsigned char* left, unsigned char* right, float* disp, float mark, unsigned int* hist, int w, int h,
                          bool host_gpu_compare);
// cost: size_d*w*h floats, [z][y][x], the volume of view `right` (0 the left view, 1 the right one) from `table` (u8
// [256][256], smx_mi_table of a histogram); slice z has label dmin + z.  left / right: the gray images, in that order for
// either view.  host_gpu_compare: the CPU twin runs as well and check_errors compares.
void compute_mi_cost(const unsigned char* table, unsigned char* left, unsigned char* right, int view, float* cost, int w, int h,
                     int size_d, int dmin, bool host_gpu_compare);
// CPU twins (cpu_twins.cpp), scalar, by the definition in include/smx.h.  The table itself is host arithmetic already
// (smx_mi_table): the twins call no log of their own.
void mi_histogramOnCPU(const unsigned char* left, const unsigned char* right, const float* disp, float mark, unsigned int* hist,
                       const int w, const int h);
void mi_costOnCPU(const unsigned char* table, const unsigned char* left, const unsigned char* right, int view, float* cost,
                  const int w, const int h, const int size_d, const int dmin);
