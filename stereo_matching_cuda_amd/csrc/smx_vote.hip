// smx_vote.hip -- region voting and 16-direction interpolation on the cross arms (the outlier refinement of Mei et al. 2011; not
// a stage of the reference: opt-in, behind LR check -> uniqueness -> speckle removal).  The definition is the comment above
// smx_vote_workspace_bytes in include/smx.h and tests/vote_ref.py, bit for bit: the votes are integers, so the order of the
// adds is free and the bits are fixed.
//
//   k_vote_round   one Jacobi round, M_k -> M_{k+1}.  A workgroup of four waves takes a tile of 64 x 4 pixels, a wave one row
//                  of it: every lane copies its pixel, a ballot finds the row's outliers, and the wave takes them in turn
//                  (no compaction, no global atomics, no order a schedule could change).  For one outlier the wave walks the
//                  rows of its vertical arm; the arms words of (y', x) are fetched 64 rows at a time, one per lane, and read
//                  back by readlane; the lanes take the row's span 64 pixels at a time with coalesced loads of M_k and add
//                  into the wave's own LDS histogram (u32 bins) with LDS atomics.  Then every lane scans and clears
//                  size_d / 64 bins, a wave-wide max of count << 9 | bin gives the largest bin among the largest counts,
//                  and the lane that owns the pixel stores the label.
//   k_vote_interp  the interpolation, or with interpolate == 0 the copy into d_out: 16 lanes per pixel, one per direction.
//                  A lane walks its direction to the first voter; the 16 lanes share the labels of the mismatch test; a
//                  max (occlusion) or min (mismatch) over the 16 lanes of a key that ends in the direction picks the lane
//                  whose candidate's bits are copied.
//   k_vote_copy    M_0 into the workspace where no round runs (iterations == 0), so that the interpolation reads a snapshot
//                  with d_out == d_disp as well.
// Arms words are read as they are (hand-made planes included): a region is cut at the image border, whatever its arms say.
//
// Workspace (from the next 256-byte boundary on): A, B: two maps of n f32, round k writes A (k even) or B (k odd).
#include <limits.h>

#include "smx_api.h"
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int VOTE_TW = 64;             // tile columns = lanes of a wave
constexpr int VOTE_TH = 4;              // tile rows = waves of a workgroup
constexpr int VOTE_DIRS = 16;          // (VOTE_MAX_D, the labels of a histogram in LDS: smx_ctx_plan.h, beside shape_ok)

// (int)v of a finite v, saturating like the hardware's conversion
__device__ inline int vote_trunc(float v) {
    return v >= 2147483648.0f ? INT_MAX : v < -2147483648.0f ? INT_MIN : (int)v;
}

// the speckle filter's rule (smx_speckle.hip speckle_counts) with vmin = (float)dmin
__device__ inline bool vote_valid(float v, float vmin) {
    if (!(fabsf(v) <= 3.402823466e38f)) return false;
    return (float)vote_trunc(v) >= vmin;
}

// the bin of a voter, or -1
__device__ inline int vote_bin(float v, float vmin, int dmin, int size_d) {
    if (!vote_valid(v, vmin)) return -1;
    const long long b = (long long)vote_trunc(v) - dmin;
    return b >= 0 && b < size_d ? (int)b : -1;
}

__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, m, 64));
    return v;
}

__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// grid: tiles, VOTE_TW * VOTE_TH threads.  in != out.
__global__ __launch_bounds__(VOTE_TW * VOTE_TH) void k_vote_round(const float* __restrict__ in, float* __restrict__ out,
                                                                  const uint32_t* __restrict__ arms, int w, int h, int dmin,
                                                                  int size_d, int tau_s, int tau_h_pct) {
    __shared__ uint32_t hist[VOTE_TH][VOTE_MAX_D];
    const int tiles_x = (w - 1) / VOTE_TW + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * VOTE_TW, y = (int)(blockIdx.x / (unsigned)tiles_x) * VOTE_TH + wave;
    uint32_t* H = hist[wave];
    for (int b = lane; b < size_d; b += 64) H[b] = 0u;
    if (y >= h) return;                 // (wave-uniform; no workgroup barrier anywhere below)
    const float vmin = (float)dmin;
    const int px = x0 + lane;
    const bool inside = px < w;
    const int64_t row = (int64_t)y * w;
    float v = 0.0f;
    uint32_t aw = 0u;
    if (inside) {
        v = in[row + px];
        aw = arms[row + px];
        out[row + px] = v;
    }
    uint64_t todo = __ballot(inside && !vote_valid(v, vmin));
    while (todo) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int x = x0 + bit;
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)aw, bit);
        const int ya = max(y - (int)((a >> 16) & 255u), 0), yb = min(y + (int)(a >> 24), h - 1);
        for (int yc = ya; yc <= yb; yc += 64) {
            const int yl = yc + lane;
            const uint32_t mine = yl <= yb ? arms[(int64_t)yl * w + x] : 0u;
            const int rows = min(64, yb - yc + 1);
            for (int j = 0; j < rows; ++j) {
                const uint32_t ar = (uint32_t)__builtin_amdgcn_readlane((int)mine, j);
                const int xa = max(x - (int)(ar & 255u), 0), xb = min(x + (int)((ar >> 8) & 255u), w - 1);
                const float* src = in + (int64_t)(yc + j) * w;
                for (int xx = xa + lane; xx <= xb; xx += 64) {
                    const int b = vote_bin(src[xx], vmin, dmin, size_d);
                    if (b >= 0) atomicAdd(&H[b], 1u);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t key = 0u, sum = 0u;
        for (int b = lane; b < size_d; b += 64) {
            const uint32_t c = __hip_atomic_load(&H[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            H[b] = 0u;
            sum += c;
            key = max(key, c << 9 | (uint32_t)b);       // (c <= 511 * 511 < 2^18, b < 2^9)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        key = wave_max_u32(key);
        sum = wave_sum_u32(sum);
        const int64_t best = key >> 9;
        if (lane == bit && (int64_t)sum > tau_s && 100 * best > (int64_t)tau_h_pct * sum)
            out[row + x] = (float)(int)((long long)dmin + (int)(key & 511u));
    }
}

__global__ __launch_bounds__(256) void k_vote_copy(const float* __restrict__ in, float* __restrict__ out, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p < n) out[p] = in[p];
}

// r | g << 8 | b << 16 of a guide pixel, and the cross aggregation's D(p, q) (smx_cross.hip load_px, cdist)
__device__ inline uint32_t vote_px(const uint8_t* g, int ch, int64_t i) {
    const uint8_t* p = g + i * ch;
    const uint32_t r = p[0];
    if (ch == 1) return r | r << 8 | r << 16;
    return r | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

__device__ inline uint32_t vote_dist(uint32_t a, uint32_t b) {
    const int d0 = abs((int)(a & 255u) - (int)(b & 255u));
    const int d1 = abs((int)((a >> 8) & 255u) - (int)((b >> 8) & 255u));
    const int d2 = abs((int)(a >> 16) - (int)(b >> 16));
    return (uint32_t)max(d0, max(d1, d2));
}

__constant__ int8_t VOTE_DX[VOTE_DIRS] = {1, 2, 1, 1, 0, -1, -1, -2, -1, -2, -1, -1, 0, 1, 1, 2};
__constant__ int8_t VOTE_DY[VOTE_DIRS] = {0, 1, 1, 2, 1, 2, 1, 1, 0, -1, -1, -2, -1, -2, -1, -1};

// grid: ceil(n / 16), 256 threads: 16 consecutive pixels, 16 lanes each.  in != out.
__global__ __launch_bounds__(256) void k_vote_interp(const float* __restrict__ in, float* __restrict__ out,
                                                     const uint8_t* __restrict__ guide, int ch, const float* __restrict__ disp_r,
                                                     int w, int h, int dmin, int size_d, int d_lr, int interpolate) {
    const int dir = threadIdx.x & 15;
    const int64_t n = (int64_t)w * h;
    int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = p < n;            // (a group past the end goes through the shuffles on the last pixel and stores nothing)
    if (!live) p = n - 1;
    const float vmin = (float)dmin;
    const float v = in[p];
    uint32_t bits = __float_as_uint(v);
    if (interpolate && !vote_valid(v, vmin)) {          // (uniform over the 16 lanes of a pixel)
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        // the candidate of this lane's direction
        const int dx = VOTE_DX[dir], dy = VOTE_DY[dir];
        bool has = false;
        float cv = 0.0f;
        int64_t cq = 0;
        for (int qx = x + dx, qy = y + dy; qx >= 0 && qx < w && qy >= 0 && qy < h; qx += dx, qy += dy) {
            const int64_t q = (int64_t)qy * w + qx;
            const float c = in[q];
            if (vote_bin(c, vmin, dmin, size_d) >= 0) { has = true; cv = c; cq = q; break; }
        }
        // the LR check's test over the labels of the range, 16 at a time
        int mm = 0;
        if (disp_r) {
            const float lim = (float)d_lr;
            for (int s = dir; s < size_d; s += VOTE_DIRS) {
                const long long d = (long long)dmin + s, xr = x + d;
                if (xr >= 0 && xr < w && fabsf((float)(int)d + disp_r[(int64_t)y * w + xr]) <= lim) mm = 1;
            }
        }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) mm |= __shfl_xor(mm, m, 16);
        // a key that orders the candidates and ends in the direction, so that equals go to the first one
        uint64_t key = 0;               // no candidate
        if (has) {
            if (mm) {
                key = (uint64_t)(255u - vote_dist(vote_px(guide, ch, cq), vote_px(guide, ch, p))) << 4 | (uint64_t)(15 - dir);
            } else {
                uint32_t u = __float_as_uint(cv == 0.0f ? 0.0f : cv);       // (-0 orders as +0)
                u = u & 0x80000000u ? ~u : u | 0x80000000u;                 // the order of the floats, as unsigned
                key = (uint64_t)u << 4 | (uint64_t)(15 - dir);
            }
            key |= 1ull << 40;
        }
        uint64_t top = key;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)top, m, 16);
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(top >> 32), m, 16);
            const uint64_t other = (uint64_t)hi << 32 | lo;
            top = other > top ? other : top;
        }
        const uint32_t cb = (uint32_t)__shfl((int)__float_as_uint(cv), 15 - (int)(top & 15u), 16);
        if (top) bits = cb;
    }
    if (live && dir == 0) out[p] = __uint_as_float(bits);
}

}  // namespace

bool vote_params_ok(const smx_vote_params* p) {
    return p && p->tau_s >= 0 && p->tau_h_pct >= 0 && p->tau_h_pct <= 99 && p->iterations >= 0 && p->iterations <= 8 &&
           (p->interpolate == 0 || p->interpolate == 1);
}

size_t vote_workspace_bytes(int w, int h) { return 255 + 2 * sizeof(float) * (size_t)w * h; }

void vote_tile(int* tw, int* th) { *tw = VOTE_TW; *th = VOTE_TH; }

int launch_region_vote(const smx_vote_params* p, const uint32_t* arms, const uint8_t* guide, int ch, const float* disp,
                       const float* disp_r, float* out, int w, int h, int dmin, int size_d, int d_lr, void* ws, hipStream_t st) {
    const size_t n = (size_t)w * h;
    float* buf[2];
    buf[0] = reinterpret_cast<float*>(align_up((size_t)ws, 256));
    buf[1] = buf[0] + n;
    const unsigned tiles = (unsigned)((size_t)((w - 1) / VOTE_TW + 1) * (size_t)((h - 1) / VOTE_TH + 1));
    const float* cur = disp;
    for (int k = 0; k < p->iterations; ++k) {
        hipLaunchKernelGGL(k_vote_round, dim3(tiles), dim3(VOTE_TW * VOTE_TH), 0, st, cur, buf[k & 1], arms, w, h, dmin, size_d,
                           p->tau_s, p->tau_h_pct);
        cur = buf[k & 1];
    }
    if (p->iterations == 0) {
        hipLaunchKernelGGL(k_vote_copy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, disp, buf[0], (uint32_t)n);
        cur = buf[0];
    }
    hipLaunchKernelGGL(k_vote_interp, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, cur, out, guide, ch, disp_r, w, h, dmin,
                       size_d, d_lr, p->interpolate);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
