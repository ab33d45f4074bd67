// adcensus.cuh -- the AD-Census matching cost, census plus absolute differences (not a stage of the reference:
// smx_main --cost adcensus).  Host pointers in / out like compute_cost (costVolume.cuh); the contract is smx_adcensus_cost's
// (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// i1 / i2: u8 [h][w][channels], channels 1 with p.colour 0 (gray), 3 or 4 with p.colour 1.  cost: size_d*w*h floats,
// [z][y][x], the volume of i1 against i2; slice z has label dmin + z.  host_gpu_compare: the CPU twin runs as well (its gray
// images from sumArraysOnHost, its tables from smx_adcensus_tables) and check_errors compares.
void compute_adcensus_cost(unsigned char* i1, unsigned char* i2, int channels, float* cost, int w, int h, int size_d, int dmin,
                           const smx_adcensus_params& p, bool host_gpu_compare);
// CPU twin (cpu_twins.cpp), scalar.  g1 / g2: the gray images the census codes come from (i1 / i2 themselves with channels 1);
// table: the SMX_ADCENSUS_TABLE_FLOATS floats of smx_adcensus_tables(&p, table) -- the twin calls no exp of its own.
void adcensus_costOnCPU(const unsigned char* i1, const unsigned char* i2, const unsigned char* g1, const unsigned char* g2,
                        int channels, float* cost, const int w, const int h, const int size_d, const int dmin,
                        const smx_adcensus_params& p, const float* table);
