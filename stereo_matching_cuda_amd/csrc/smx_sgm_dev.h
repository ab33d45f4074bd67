// smx_sgm_dev.h -- what the path walkers of smx_sgm.hip (constant penalties) and smx_scanline.hip (colour-adaptive penalties)
// share on the device: the planes' argument struct, the pack and select kernels around the walks, and the register helpers of
// a step (the packed loads of a lane, the DPP wave shifts, the wave minimum).  The layout of the planes and the scheme of a
// walk are described at the top of smx_sgm.hip.  The kernels sit in an anonymous namespace: each of the two files launches
// its own copy under the one name.
#pragma once
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int SGM_BIG = 1 << 20;        // "no such disparity": above every path cost, far from overflow with + p1
constexpr int SGM_TILE = 64;            // pixels (and disparities) of a pack / select tile
constexpr int SGM_WAVES = 4;            // paths per workgroup of the path kernels

struct SgmArgs {
    const float* cost[2];    // the views of this launch (nviews of them)
    int64_t* keys[2];
    float* agg[2];
    float* nbr[2];
    float* uq[2];
    uint8_t* c8[2];
    uint16_t* s16[2];
    int w, h, size_d, dp, p1, p2, xtiles;
};

__device__ inline int clamp_cost(float c) { return c >= 0.0f ? (c <= 255.0f ? (int)c : 255) : 0; }

// grid (xtiles * h, dp / 64, nviews), 256 threads
__global__ __launch_bounds__(256) void k_sgm_pack(const SgmArgs a) {
    __shared__ alignas(4) uint8_t tile[SGM_TILE][SGM_TILE + 4];     // [x][d]; 68 bytes = 17 words a row
    const int v = blockIdx.z;
    const int y = (int)(blockIdx.x / (unsigned)a.xtiles);
    const int x0 = (int)(blockIdx.x % (unsigned)a.xtiles) * SGM_TILE;
    const int d0 = (int)blockIdx.y * SGM_TILE;
    const int64_t n = (int64_t)a.w * a.h, row = (int64_t)y * a.w;
    const float* cost = a.cost[v];
    {
        const int x = threadIdx.x & 63, dg = threadIdx.x >> 6;
#pragma unroll 4
        for (int i = 0; i < SGM_TILE / 4; ++i) {
            const int d = d0 + dg + 4 * i;
            int c = 0;
            if (d < a.size_d && x0 + x < a.w) c = clamp_cost(cost[(int64_t)d * n + row + x0 + x]);
            tile[x][dg + 4 * i] = (uint8_t)c;
        }
    }
    __syncthreads();
    const int dq = threadIdx.x & 15;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = (int)(threadIdx.x >> 4) + 16 * i;
        if (x0 + x >= a.w) continue;
        const uint32_t four = *reinterpret_cast<const uint32_t*>(&tile[x][4 * dq]);
        *reinterpret_cast<uint32_t*>(a.c8[v] + (row + x0 + x) * a.dp + d0 + 4 * dq) = four;
    }
}

// ---- one step of a path, all in registers ----------------------------------------------------------------------------
template <int VPL> struct Pk;           // the VPL costs (u8) and the VPL sums (u16) of a lane as one load each
template <> struct Pk<1> { typedef uint8_t C; typedef uint16_t S; };
template <> struct Pk<2> { typedef uint16_t C; typedef uint32_t S; };
template <> struct Pk<4> { typedef uint32_t C; typedef uint2 S; };

template <int VPL> __device__ inline void unpack_c(typename Pk<VPL>::C c, int* out) {
    const uint32_t u = (uint32_t)c;
#pragma unroll
    for (int j = 0; j < VPL; ++j) out[j] = (int)((u >> (8 * j)) & 0xFFu);
}
__device__ inline void unpack_s(uint16_t s, int* out) { out[0] = s; }
__device__ inline void unpack_s(uint32_t s, int* out) { out[0] = (int)(s & 0xFFFFu); out[1] = (int)(s >> 16); }
__device__ inline void unpack_s(uint2 s, int* out) {
    out[0] = (int)(s.x & 0xFFFFu); out[1] = (int)(s.x >> 16); out[2] = (int)(s.y & 0xFFFFu); out[3] = (int)(s.y >> 16);
}
__device__ inline void pack_s(const int* in, uint16_t* s) { *s = (uint16_t)in[0]; }
__device__ inline void pack_s(const int* in, uint32_t* s) { *s = ((uint32_t)in[0] & 0xFFFFu) | ((uint32_t)in[1] << 16); }
__device__ inline void pack_s(const int* in, uint2* s) {
    s->x = ((uint32_t)in[0] & 0xFFFFu) | ((uint32_t)in[1] << 16);
    s->y = ((uint32_t)in[2] & 0xFFFFu) | ((uint32_t)in[3] << 16);
}

// lane i <- lane i - 1 (lane 0 <- fill), lane i <- lane i + 1 (lane 63 <- fill): DPP wave_shr:1 / wave_shl:1
__device__ inline int from_lane_below(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xF, 0xF, false); }
__device__ inline int from_lane_above(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x130, 0xF, 0xF, false); }
// the minimum over the wave, uniform: rotations inside each row of 16 lanes (row_ror:1, 2, 4, 8), then the four rows
__device__ inline int wave_min(int x) {
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x121, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x122, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x124, 0xF, 0xF, false));
    x = min(x, __builtin_amdgcn_update_dpp(x, x, 0x128, 0xF, 0xF, false));
    return min(min(__builtin_amdgcn_readlane(x, 0), __builtin_amdgcn_readlane(x, 16)),
               min(__builtin_amdgcn_readlane(x, 32), __builtin_amdgcn_readlane(x, 48)));
}

// grid (xtiles * h, nviews), 256 threads, dynamic LDS: 64 rows of dp + 2 u16
__global__ __launch_bounds__(256) void k_sgm_select(const SgmArgs a) {
    extern __shared__ uint32_t s_tile[];
    const int v = blockIdx.y;
    const int y = (int)(blockIdx.x / (unsigned)a.xtiles);
    const int x0 = (int)(blockIdx.x % (unsigned)a.xtiles) * SGM_TILE;
    const int npx = min(SGM_TILE, a.w - x0);
    const int64_t n = (int64_t)a.w * a.h, row = (int64_t)y * a.w;
    const int half = a.dp / 2, stride = half + 1;        // u32 words of a pixel in S16 and in the tile (odd: no conflicts)
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.s16[v] + (row + x0) * a.dp);
    for (int e = threadIdx.x; e < npx * half; e += 256) {
        const int px = e / half, k = e - px * half;
        s_tile[px * stride + k] = src[e];
    }
    __syncthreads();
    const uint16_t* t16 = reinterpret_cast<const uint16_t*>(s_tile);
    const int x = threadIdx.x & 63;
    if (x >= npx) return;
    const uint16_t* mine = t16 + x * (2 * stride);
    if (a.agg[v]) {
        float* out = a.agg[v] + row + x0 + x;
        for (int d = threadIdx.x >> 6; d < a.size_d; d += 4) out[(int64_t)d * n] = (float)mine[d];
    }
    if (threadIdx.x >= 64) return;
    int m = mine[0], z = 0;
    for (int d = 1; d < a.size_d; ++d) {
        const int s = mine[d];
        const bool take = s <= m;             // the last slice of equal costs wins
        m = take ? s : m;
        z = take ? d : z;
    }
    a.keys[v][row + x0 + x] = pack_key((float)m, (uint32_t)z);
    if (a.nbr[v]) {
        float* nb = a.nbr[v] + row + x0 + x;
        nb[0] = z > 0 ? (float)mine[z - 1] : __builtin_nanf("");
        nb[n] = z + 1 < a.size_d ? (float)mine[z + 1] : __builtin_nanf("");
        nb[2 * n] = (float)mine[a.size_d - 1];
    }
    if (a.uq[v]) {
        // the uniqueness state of one run over the whole range (smx_common.h WtaRunUq; exact: S are integers)
        WtaRunUq r;
        for (int d = 0; d < a.size_d; ++d) r.step((float)mine[d], (uint32_t)d);
        float* u = a.uq[v] + row + x0 + x;
        u[0] = r.sec;
        u[n] = r.rest;
        u[2 * n] = r.last;
    }
}

// the launches around the walks, with their geometry
inline size_t sgm_plane_bytes(int w, int h, int size_d) { return align_up((size_t)w * h * (size_t)sgm_padded_d(size_d), 256); }
inline size_t sgm_select_lds(int dp) { return (size_t)SGM_TILE * (dp / 2 + 1) * sizeof(uint32_t); }

}  // namespace
}  // namespace smx
