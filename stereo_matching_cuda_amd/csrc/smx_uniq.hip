// Uniqueness (peak-ratio) filtering of a disparity map from the second-best cost the WTA passes keep (smx_common.h WtaRunUq,
// uniq_rejects).  Not a stage of the reference.  Contract: include/smx.h, smx_dev_uniqueness.
//
// One lane per pixel, every access coalesced: 8 B of key, 4 B of sec and 4 B of map in, 4 B (8 B with the margins) out.
// A lane reads and writes its own pixel only, so out == disp is allowed.
//
// Must be compiled with -ffp-contract=off.
#include "smx_launch.h"

namespace smx {
namespace {

// the speckle filter's validity rule (smx_speckle.hip speckle_counts): finite, and fill_occlusion's test against vmin
__device__ inline bool uniq_counts(float v, float vmin) {
    if (!(fabsf(v) <= 3.402823466e38f)) return false;       // NaN, +-inf
    const float t = v >= 2147483648.0f ? 2147483648.0f : v < -2147483648.0f ? -2147483648.0f : (float)(int)v;
    return t >= vmin;
}

__global__ __launch_bounds__(256) void k_uniqueness(const int64_t* __restrict__ keys, const float* __restrict__ sec,
                                                    const float* disp, float* out, float* __restrict__ margin, int64_t n,
                                                    float ratio, float vmin, float new_val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float mg;
    const bool rejected = uniq_rejects(keys[i], sec[i], ratio, &mg);
    const float d = disp[i];
    out[i] = rejected && uniq_counts(d, vmin) ? new_val : d;
    if (margin) margin[i] = mg;
}

}  // namespace

int launch_uniqueness(float ratio, const int64_t* keys, const float* uq, const float* disp, float* out, float* margin, int64_t n,
                      float vmin, float new_val, hipStream_t st) {
    const int64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return fail(SMX_E_ARG, "smx_dev_uniqueness: %lld pixels are too many", (long long)n);
    hipLaunchKernelGGL(k_uniqueness, dim3((unsigned)blocks), dim3(256), 0, st, keys, uq, disp, out, margin, n, ratio, vmin, new_val);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
