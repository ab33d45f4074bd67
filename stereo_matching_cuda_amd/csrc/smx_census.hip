// Census transform and Hamming matching cost (Zabih & Woodfill; the census half of AD-Census).  Not a stage of the
// reference: an opt-in alternative to costVolume.cu's truncated absolute difference + x-gradient.  It depends only on the
// ORDER of the gray values in a window, so a strictly increasing change of one image's intensities leaves the volume
// untouched.  Contract (bit numbering, replicate clamp, border cost, slice placement): include/smx.h.
//
// k_census: one workgroup per 64 x 8 tile of one image, four waves, two pixels per lane.  The tile plus its (rx, ry) halo
// is staged in LDS with the coordinates clamped to the image, so the window loop reads LDS only.
//
// k_census_cost_pair: a pure store stream (2 * slices * w * h floats).  A workgroup owns 256 columns of one row of one
// view and CC_Z consecutive slices.  The 256 + CC_Z - 1 codes of the other view those slices touch are staged in LDS
// (positions outside the image hold a marker with bit 63 set, which no code has: nbits <= 62); a lane keeps its own code
// in two VGPRs and does, per slice, one 8-byte LDS read, two xor, two popcounts, a min and one coalesced 4-byte store.
// Plain stores: non-temporal ones were measured 38 % slower for the kernel and 6 % for the pair step.
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int CEN_TW = 64, CEN_TH = 8, CEN_THREADS = 256;
constexpr int CEN_RX = 4, CEN_RY = 3;                       // the largest window
constexpr int CC_COLS = 256;                                // columns (= lanes) of a cost workgroup
constexpr int CC_Z = 16;                                    // slices of a cost workgroup
constexpr uint64_t CC_OUTSIDE = 0x8000000000000000ull;      // the partner lies outside the image

// grid (tiles_x * tiles_y, nimages)
__global__ __launch_bounds__(CEN_THREADS) void k_census(const uint8_t* __restrict__ img, uint64_t* __restrict__ code,
                                                        int w, int h, int rx, int ry) {
    __shared__ uint8_t tile[(CEN_TH + 2 * CEN_RY) * (CEN_TW + 2 * CEN_RX)];
    const int tiles_x = (w + CEN_TW - 1) / CEN_TW;
    const int x0 = (int)(blockIdx.x % tiles_x) * CEN_TW, y0 = (int)(blockIdx.x / tiles_x) * CEN_TH;
    const int64_t n = (int64_t)w * h;
    const uint8_t* I = img + (int64_t)blockIdx.y * n;
    const int hw = CEN_TW + 2 * rx, hh = CEN_TH + 2 * ry;
    for (int i = threadIdx.x; i < hw * hh; i += CEN_THREADS) {
        const int hy = i / hw, hx = i - hy * hw;
        const int y = min(max(y0 - ry + hy, 0), h - 1), x = min(max(x0 - rx + hx, 0), w - 1);
        tile[i] = I[(int64_t)y * w + x];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63;
    if (x0 + tx >= w) return;
#pragma unroll
    for (int j = 0; j < CEN_TH / 4; ++j) {
        const int ty = (int)(threadIdx.x >> 6) + 4 * j;
        if (y0 + ty >= h) continue;
        const uint8_t* ctr = tile + (ty + ry) * hw + (tx + rx);
        const uint32_t c = ctr[0];
        uint64_t bits = 0;
        int k = 0;
        for (int dy = -ry; dy <= ry; ++dy)
            for (int dx = -rx; dx <= rx; ++dx) {
                if (dy == 0 && dx == 0) continue;
                bits |= (uint64_t)(ctr[dy * hw + dx] < c) << k;
                ++k;
            }
        code[(int64_t)blockIdx.y * n + (int64_t)(y0 + ty) * w + (x0 + tx)] = bits;
    }
}

struct CensusCostArgs {
    const uint64_t* code;    // [2][h][w]: left, right
    float* cost[2];          // the views this launch writes (nviews of them)
    int dmin[2];
    int view[2];             // 0 left, 1 right
    int w, h, s_begin, s_end, t, xblocks;
};

// grid (xblocks * h, ceil(slices / CC_Z), nviews)
__global__ __launch_bounds__(CC_COLS) void k_census_cost_pair(const CensusCostArgs a) {
    __shared__ uint64_t other[CC_COLS + CC_Z - 1];
    const int v = blockIdx.z;
    const int y = (int)(blockIdx.x / (unsigned)a.xblocks);
    const int x0 = (int)(blockIdx.x % (unsigned)a.xblocks) * CC_COLS;
    const int z0 = a.s_begin + (int)blockIdx.y * CC_Z;
    const int nz = min(CC_Z, a.s_end - z0);
    const int64_t n = (int64_t)a.w * a.h, row = (int64_t)y * a.w;
    const uint64_t* own_codes = a.code + (int64_t)a.view[v] * n + row;
    const uint64_t* oth_codes = a.code + (int64_t)(1 - a.view[v]) * n + row;
    // other[j] = the other view's code at x0 + d(z0) + j, d(z) = dmin + z
    const int64_t p0 = (int64_t)x0 + a.dmin[v] + z0;
    for (int j = threadIdx.x; j < CC_COLS + nz - 1; j += CC_COLS) {
        const int64_t p = p0 + j;
        other[j] = (p >= 0 && p < a.w) ? oth_codes[p] : CC_OUTSIDE;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x >= a.w) return;
    const uint64_t own = own_codes[x];
    const uint32_t t = (uint32_t)a.t;
    float* out = a.cost[v] + (int64_t)(z0 - a.s_begin) * n + row + x;
#pragma unroll 4
    for (int z = 0; z < nz; ++z) {
        const uint64_t d = own ^ other[threadIdx.x + z];
        const uint32_t pc = (uint32_t)__popcll(d);
        out[(int64_t)z * n] = (float)((int64_t)d < 0 ? t : min(pc, t));
    }
}

}  // namespace

int launch_census(int rx, int ry, const uint8_t* img, uint64_t* code, int w, int h, int nimages, hipStream_t st) {
    const long long tiles = (long long)((w + CEN_TW - 1) / CEN_TW) * ((h + CEN_TH - 1) / CEN_TH);
    if (tiles > 0x7FFFFFFFll || nimages > 65535)
        return fail(SMX_E_ARG, "smx_dev_census: %d images of %d x %d are too many tiles", nimages, w, h);
    hipLaunchKernelGGL(k_census, dim3((unsigned)tiles, (unsigned)nimages), dim3(CEN_THREADS), 0, st, img, code, w, h, rx, ry);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_census_cost_pair(int t, const uint64_t* code, float* cost_l, float* cost_r, int w, int h, int dminl, int dminr,
                            int s_begin, int s_end, hipStream_t st) {
    if (s_end <= s_begin) return SMX_OK;
    CensusCostArgs a;
    a.code = code;
    int nviews = 0;
    if (cost_l) { a.cost[nviews] = cost_l; a.dmin[nviews] = dminl; a.view[nviews] = 0; ++nviews; }
    if (cost_r) { a.cost[nviews] = cost_r; a.dmin[nviews] = dminr; a.view[nviews] = 1; ++nviews; }
    for (int v = nviews; v < 2; ++v) { a.cost[v] = nullptr; a.dmin[v] = 0; a.view[v] = 0; }
    a.w = w; a.h = h; a.s_begin = s_begin; a.s_end = s_end; a.t = t;
    a.xblocks = (w + CC_COLS - 1) / CC_COLS;
    const long long rows = (long long)a.xblocks * h;
    const long long zblocks = ((long long)s_end - s_begin + CC_Z - 1) / CC_Z;
    if (rows > 0x7FFFFFFFll || zblocks > 65535)
        return fail(SMX_E_ARG, "smx_dev_census_cost_pair: %d x %d with %d slices is too many workgroups", w, h, s_end - s_begin);
    hipLaunchKernelGGL(k_census_cost_pair, dim3((unsigned)rows, (unsigned)zblocks, (unsigned)nviews), dim3(CC_COLS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
