// Weighted-median refinement of a disparity map (Hosni et al., "Fast Cost-Volume Filtering for Visual Correspondence
// and Beyond", the bilateral weighted median that follows the scan-line fill).  Not a stage of the reference: a new
// stage behind occlusion.cu's fill_occlusion.  Contract (weights, sample rule, tie rule, selection): include/smx.h.
//
// One workgroup per 64 x 8 output tile, four waves.  The tile plus its radius halo is staged in LDS as one packed word
// per pixel (label index << 8 | gray), so a window sample is one ds_read_b32.  The selected pixels of the tile are
// compacted into a list first: a wave takes 64 entries of the list at a time, so in "occluded" mode lanes and waves
// without a selected pixel do no window work, and a tile without one stages nothing.  The median is exact and two-level:
// pass 1 histograms buckets of B = 2^shift labels (B^2 >= size_d, so B <= 64 bins for size_d <= 4096) and finds the
// bucket that holds the median, pass 2 histograms the B labels of that bucket.  A lane's bins live in its own LDS
// column (bin*64 + lane: bank = lane mod 32, no conflicts, no contention for the ds_add).  Weights are integers, so
// the sums are exact in any order.
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int WMF_TW = 64;                      // tile columns = lanes of a wave
constexpr int WMF_TH = 8;                       // tile rows
constexpr int WMF_WAVES = 4;
constexpr int WMF_THREADS = 64 * WMF_WAVES;
constexpr uint32_t WMF_NONE = 0xFFFFFu;         // label field of a sample that counts for nothing
constexpr int WMF_NSPATIAL = 2 * 15 * 15 + 1;   // ws[0 .. 2 r^2] at the largest radius

struct WmfArgs {
    const uint8_t* guide;
    const float* disp;
    const float* select;
    float* out;
    int w, h, dmin, size_d, r, shift;
    uint16_t ws[WMF_NSPATIAL + 1];
    uint16_t wc[256];
};

// label index of a disparity value: v - dmin if v is an integer in [dmin, dmin + size_d), else WMF_NONE
__device__ inline uint32_t wmf_label(float v, int dmin, int size_d) {
    if (!(fabsf(v) < 2147483648.0f)) return WMF_NONE;     // NaN, +-inf, beyond int
    const int iv = (int)v;
    if ((float)iv != v) return WMF_NONE;                  // a fraction (-0.0 is the integer 0)
    const long long k = (long long)iv - dmin;
    return (k >= 0 && k < size_d) ? (uint32_t)k : WMF_NONE;
}

// (int)select < dmin, defined for every float: NaN and +-inf select nothing
__device__ inline bool wmf_selected(const float* select, size_t i, int dmin) {
    if (!select) return true;
    const float s = select[i];
    if (!(fabsf(s) <= 3.402823466e38f)) return false;
    return trunc((double)s) < (double)dmin;
}

__global__ __launch_bounds__(WMF_THREADS) void k_weighted_median(const WmfArgs a) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t row_count[WMF_TH];
    const int r = a.r, hw = WMF_TW + 2 * r, hh = WMF_TH + 2 * r;
    const int shift = a.shift, nb = 1 << shift;
    uint32_t* halo = lds;                                      // hw * hh packed samples
    uint32_t* wct = halo + hw * hh;                            // wct[255 + t] = wc[|t|], t = g(q) - g(p)
    uint32_t* wsl = wct + 512;                                 // wsl[k] = ws[k], k = dx^2 + dy^2 <= 2 r^2
    uint32_t* hist = wsl + WMF_NSPATIAL + 1;                   // per wave nb * 64 bins
    uint16_t* list = (uint16_t*)(hist + WMF_WAVES * nb * 64);  // selected pixels of the tile: ty * 64 + tx

    const int tiles_x = (a.w + WMF_TW - 1) / WMF_TW;
    const int x0 = (int)(blockIdx.x % tiles_x) * WMF_TW, y0 = (int)(blockIdx.x / tiles_x) * WMF_TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // 1. selection: pixels that are not filtered are copied; the selected ones go into the list in raster order
    uint64_t mask[WMF_TH / WMF_WAVES];
#pragma unroll
    for (int j = 0; j < WMF_TH / WMF_WAVES; ++j) {
        const int ty = wave + j * WMF_WAVES, x = x0 + lane, y = y0 + ty;
        bool sel = false;
        if (x < a.w && y < a.h) {
            const size_t i = (size_t)y * a.w + x;
            sel = wmf_selected(a.select, i, a.dmin);
            if (!sel) a.out[i] = a.disp[i];
        }
        mask[j] = __ballot(sel);
        if (lane == 0) row_count[ty] = (uint32_t)__popcll(mask[j]);
    }
    __syncthreads();
    int n_list = 0;
#pragma unroll
    for (int j = 0; j < WMF_TH; ++j) n_list += (int)row_count[j];
    if (n_list == 0) return;                                   // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < WMF_TH / WMF_WAVES; ++j) {
        const int ty = wave + j * WMF_WAVES;
        int off = 0;
        for (int k = 0; k < ty; ++k) off += (int)row_count[k];
        const uint64_t m = mask[j];
        if ((m >> lane) & 1)
            list[off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] =
                (uint16_t)(ty * WMF_TW + lane);
    }

    // 2. the tile with its halo (outside the image: samples that count for nothing), the range table, empty bins
    for (int i = threadIdx.x; i < hw * hh; i += WMF_THREADS) {
        const int hy = i / hw, hx = i - hy * hw;
        const int x = x0 - r + hx, y = y0 - r + hy;
        uint32_t v = WMF_NONE << 8;
        if (x >= 0 && x < a.w && y >= 0 && y < a.h) {
            const size_t g = (size_t)y * a.w + x;
            v = (wmf_label(a.disp[g], a.dmin, a.size_d) << 8) | a.guide[g];
        }
        halo[i] = v;
    }
    for (int i = threadIdx.x; i < 511; i += WMF_THREADS) wct[i] = a.wc[i < 255 ? 255 - i : i - 255];
    for (int i = threadIdx.x; i <= 2 * r * r; i += WMF_THREADS) wsl[i] = a.ws[i];
    for (int i = threadIdx.x; i < WMF_WAVES * nb * 64; i += WMF_THREADS) hist[i] = 0;
    __syncthreads();

    // 3. 64 list entries per wave and step; both passes walk the window in the same uniform order, so the spatial
    //    weight is a scalar per sample
    uint32_t* bins = hist + wave * nb * 64 + lane;
    const int bsh = 8 + shift;
    for (int c = wave * 64; c < n_list; c += WMF_WAVES * 64) {
        const bool act = c + lane < n_list;
        // the window loops run for the whole wave: a lane's spatial weights of a row are read by every lane
        // (v_readlane), so no lane may skip the load; a lane without a pixel adds weight 0 to its own bins
        const uint32_t lim = act ? (uint32_t)a.size_d << 8 : 0u;
        const int e = list[act ? c + lane : c];
        const int ty = e >> 6, tx = e & 63;
        const uint32_t* ctr = halo + (ty + r) * hw + (tx + r);
        const uint32_t* wrow = wct + 255 - (ctr[0] & 0xFF);
        uint32_t total = 0;
        {
            // branch-free: a sample that counts for nothing adds 0 to the last bin.  The four range weights of a step
            // are read before its four adds (the compiler cannot move a table read across an LDS add)
            auto bin1 = [&](uint32_t q) { return bins + min(q >> bsh, (uint32_t)(nb - 1)) * 64; };
            auto wt1 = [&](uint32_t q, uint32_t wv, int sw) { return __umul24(q < lim ? (uint32_t)sw : 0u, wv); };
            for (int dy = -r; dy <= r; ++dy) {
                const uint32_t* row = ctr + dy * hw - r;
                const int sw = wsl[lane <= 2 * r ? dy * dy + (lane - r) * (lane - r) : 0];   // lane j: weight of dx = j - r
                int j = 0;
                for (; j + 3 <= 2 * r; j += 4) {
                    const uint32_t q0 = row[j], q1 = row[j + 1], q2 = row[j + 2], q3 = row[j + 3];
                    const uint32_t v0 = wrow[q0 & 0xFF], v1 = wrow[q1 & 0xFF], v2 = wrow[q2 & 0xFF], v3 = wrow[q3 & 0xFF];
                    const uint32_t t0 = wt1(q0, v0, __builtin_amdgcn_readlane(sw, j));
                    const uint32_t t1 = wt1(q1, v1, __builtin_amdgcn_readlane(sw, j + 1));
                    const uint32_t t2 = wt1(q2, v2, __builtin_amdgcn_readlane(sw, j + 2));
                    const uint32_t t3 = wt1(q3, v3, __builtin_amdgcn_readlane(sw, j + 3));
                    total += t0 + t1 + t2 + t3;
                    atomicAdd(bin1(q0), t0);
                    atomicAdd(bin1(q1), t1);
                    atomicAdd(bin1(q2), t2);
                    atomicAdd(bin1(q3), t3);
                }
                for (; j <= 2 * r; ++j) {
                    const uint32_t q = row[j], t = wt1(q, wrow[q & 0xFF], __builtin_amdgcn_readlane(sw, j));
                    total += t;
                    atomicAdd(bin1(q), t);
                }
            }
        }
        // the bucket that holds the median (every lane reads and clears its column)
        uint32_t cum = 0, below = 0;
        int jb = -1;
        for (int j = 0; j < nb; ++j) {
            const uint32_t v = bins[j * 64];
            bins[j * 64] = 0;
            if (jb < 0 && 2 * (cum + v) >= total) { jb = j; below = cum; }
            cum += v;
        }
        // the labels of that bucket (a sample that counts for nothing never matches it, nor does any sample of a lane
        // without a pixel or with total 0)
        const uint32_t jq = act && total ? (uint32_t)jb : 0xFFFFFFFFu;
        if (__any(jq != 0xFFFFFFFFu)) {
            const uint32_t fm = (uint32_t)(nb - 1);
            auto bin2 = [&](uint32_t q) { return bins + ((q >> 8) & fm) * 64; };
            auto wt2 = [&](uint32_t q, uint32_t wv, int sw) { return __umul24((q >> bsh) == jq ? (uint32_t)sw : 0u, wv); };
            for (int dy = -r; dy <= r; ++dy) {
                const uint32_t* row = ctr + dy * hw - r;
                const int sw = wsl[lane <= 2 * r ? dy * dy + (lane - r) * (lane - r) : 0];
                int j = 0;
                for (; j + 3 <= 2 * r; j += 4) {
                    const uint32_t q0 = row[j], q1 = row[j + 1], q2 = row[j + 2], q3 = row[j + 3];
                    const uint32_t v0 = wrow[q0 & 0xFF], v1 = wrow[q1 & 0xFF], v2 = wrow[q2 & 0xFF], v3 = wrow[q3 & 0xFF];
                    const uint32_t t0 = wt2(q0, v0, __builtin_amdgcn_readlane(sw, j));
                    const uint32_t t1 = wt2(q1, v1, __builtin_amdgcn_readlane(sw, j + 1));
                    const uint32_t t2 = wt2(q2, v2, __builtin_amdgcn_readlane(sw, j + 2));
                    const uint32_t t3 = wt2(q3, v3, __builtin_amdgcn_readlane(sw, j + 3));
                    atomicAdd(bin2(q0), t0);
                    atomicAdd(bin2(q1), t1);
                    atomicAdd(bin2(q2), t2);
                    atomicAdd(bin2(q3), t3);
                }
                for (; j <= 2 * r; ++j) {
                    const uint32_t q = row[j];
                    atomicAdd(bin2(q), wt2(q, wrow[q & 0xFF], __builtin_amdgcn_readlane(sw, j)));
                }
            }
        }
        // the label inside that bucket
        cum = below;
        int kf = -1;
        for (int j = 0; j < nb; ++j) {
            const uint32_t v = bins[j * 64];
            bins[j * 64] = 0;
            cum += v;
            if (kf < 0 && 2 * cum >= total) kf = j;
        }
        if (act) {
            const size_t i = (size_t)(y0 + ty) * a.w + (x0 + tx);
            a.out[i] = total ? (float)(a.dmin + (jb << shift) + kf) : a.disp[i];
        }
    }
}

size_t wmf_lds_bytes(int r, int shift) {
    return (size_t)(WMF_TW + 2 * r) * (WMF_TH + 2 * r) * 4 + 512 * 4 + (WMF_NSPATIAL + 1) * 4 +
           (size_t)WMF_WAVES * (64 << shift) * 4 + WMF_TW * WMF_TH * 2;
}

}  // namespace

int wmf_bucket_shift(int size_d) {
    int s = 0;
    while ((1 << (2 * s)) < size_d) ++s;
    return s;
}

int launch_weighted_median(int radius, const uint16_t* ws, const uint16_t* wc, const uint8_t* guide, const float* disp,
                           const float* select, float* out, int w, int h, int dmin, int size_d, hipStream_t st) {
    static LdsLimitOnce lds_limit;
    WmfArgs a;
    a.guide = guide; a.disp = disp; a.select = select; a.out = out;
    a.w = w; a.h = h; a.dmin = dmin; a.size_d = size_d; a.r = radius; a.shift = wmf_bucket_shift(size_d);
    for (int k = 0; k <= WMF_NSPATIAL; ++k) a.ws[k] = k <= 2 * radius * radius ? ws[k] : 0;
    for (int t = 0; t < 256; ++t) a.wc[t] = wc[t];
    const size_t lds = wmf_lds_bytes(radius, a.shift);
    SMX_HIP(lds_limit.ensure((const void*)k_weighted_median, (int)wmf_lds_bytes(15, 6)));
    const long long tiles = (long long)((w + WMF_TW - 1) / WMF_TW) * ((h + WMF_TH - 1) / WMF_TH);
    if (tiles > 0x7FFFFFFFll) return fail(SMX_E_ARG, "smx_dev_weighted_median: %d x %d is too many tiles", w, h);
    hipLaunchKernelGGL(k_weighted_median, dim3((unsigned)tiles), dim3(WMF_THREADS), lds, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
