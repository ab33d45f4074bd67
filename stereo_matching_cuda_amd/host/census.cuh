// census.cuh -- the census / Hamming matching cost (not a stage of the reference: smx_main --cost census).
// Host pointers in / out like compute_cost (costVolume.cuh); the contract is smx_census_cost's (include/smx.h).
#pragma once
#include "SystemIncludes.h"
#include "helpers.cuh"

// cost: size_d*w*h floats, [z][y][x], the volume of i1 against i2; slice z has label dmin + z.
void compute_census_cost(unsigned char* i1, unsigned char* i2, float* cost, int w, int h, int size_d, int dmin,
                         const smx_census_params& p);
