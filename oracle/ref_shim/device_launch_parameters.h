/* Empty on purpose: cuda_runtime.h of this directory declares threadIdx / blockIdx / blockDim / gridDim. */
#pragma once
