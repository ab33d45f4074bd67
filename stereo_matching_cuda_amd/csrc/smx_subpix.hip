// Sub-pixel disparity from the winner's neighbouring aggregated costs (not a stage of the reference; opt-in, after
// smx_dev_finish_pair).  The neighbours come from the WTA passes of the _nbr aggregation entries (smx_common.h
// WtaRunNbr, nbr_merge); the offset is subpixel_delta (smx_common.h), so the host helper smx_subpixel_delta and numpy
// float32 give the same bits.
#include "smx_launch.h"

namespace smx {

// One lane per pixel of both views: i < n left, i >= n right.  keys / dmap [2][h][w], nbr [2][3][h][w] (lo, hi, last).
// sub = dmap + delta; sub_filled (left view, optional) = sub where the LR check kept the pixel, filled where it did not --
// fill_occlusion's test, (int)occlusion < dminl, defined for every float (NaN and +-inf count as kept).
__global__ __launch_bounds__(256) void k_subpixel_pair(int mode, const int64_t* __restrict__ keys, const float* __restrict__ nbr,
                                                       const float* __restrict__ dmap, const float* __restrict__ occlusion,
                                                       const float* __restrict__ filled, size_t n, int dminl,
                                                       float* __restrict__ sub, float* __restrict__ sub_filled) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n) return;
    const size_t v = i >= n ? 1 : 0, j = i - v * n;
    const int64_t key = keys[i];
    float delta = 0.0f;
    if (key != KEY_IDENTITY) {
        float c0;
        uint32_t s;
        unpack_key(key, &c0, &s);
        const float* const st = nbr + v * 3 * n;
        delta = subpixel_delta(mode, c0, st[j], st[n + j]);
    }
    const float d = dmap[i] + delta;
    sub[i] = d;
    if (sub_filled && v == 0) {
        const float o = occlusion[j];
        const bool dropped = fabsf(o) <= 3.402823466e38f && trunc((double)o) < (double)dminl;
        sub_filled[j] = dropped ? filled[j] : d;
    }
}

int launch_subpixel_pair(int mode, const int64_t* keys, const float* nbr, const float* dmap, const float* occlusion,
                         const float* filled, int w, int h, int dminl, float* sub, float* sub_filled, hipStream_t st) {
    const size_t n = (size_t)w * h;
    hipLaunchKernelGGL(k_subpixel_pair, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st, mode, keys, nbr, dmap, occlusion,
                       filled, n, dminl, sub, sub_filled);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
