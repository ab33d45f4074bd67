// Semi-global matching (Hirschmueller 2008) as an opt-in aggregation of a cost volume.  Not a stage of the reference.
// Contract (clamp, directions, recurrence, tie rule, outputs): include/smx.h, smx_dev_sgm_wta_pair.
//
// The public layout [z][y][x] is the wrong one for a recurrence that needs every disparity of a pixel at each step, so the
// call works on two planes of the workspace per view, both [y][x][Dp] with Dp = size_d rounded up to 64:
//   C8  u8   the clamped integer costs            (k_sgm_pack: 64 x 64 tiles through LDS, both sides coalesced)
//   S16 u16  the sum of the path costs so far     (S <= 8 * (255 + 4095) = 34800)
//
// Paths.  ONE WAVE walks one path and holds all disparities of the path's current pixel in registers: lane l owns the VPL
// consecutive disparities l * VPL .. (VPL = 1, 2, 4 for Dp = 64, 128, <= 256), so a pixel's costs are one 1/2/4-byte load
// per lane and its S one 2/4/8-byte load and store, contiguous over the wave.  L(d - 1) and L(d + 1) are the lane's own
// registers except at the lane's two ends, which come from the neighbouring lanes by one DPP wave shift each; the minimum
// over d is a DPP rotate-reduction inside each row of 16 lanes and four v_readlane, so it ends in a scalar register.  No
// LDS, no barrier, no atomics: a wave never waits for another one.  (The issue's sketch puts a wave on 64 disparities and
// joins the waves of a pixel through LDS and a barrier per step; one wave per path takes that barrier out of the chain.)
// Disparities >= size_d hold SGM_BIG in the registers, which loses every min, and add 0 to S.
//   k_sgm_rows: a wave per image row, left to right (stores S), then right to left (adds).
//   k_sgm_cols: a wave per start column x0; at step s it is in row s (or h - 1 - s) and column (x0 + dx * s) mod w, and it
//               restarts with L = C where the column wraps: that is where a diagonal enters from the side border.  dx and
//               the row direction are kernel arguments (scalar registers), so two kernels make the eight paths.
// The launches follow each other on the one stream: every pass touches every cell, each cell from exactly one wave.
// The next pixel's costs and S are loaded before the current pixel's reduction, so that the chain of a path is the
// arithmetic of a step and not a memory latency.
//
// k_sgm_select: a workgroup per 64 pixels of a row stages their S (one contiguous piece of S16) in LDS, writes the f32
// volume [z][y][x] from it (lanes along x: coalesced) and lets one lane per pixel run the tie rule over ascending d.
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

// L <- the path costs of the next pixel of the path from those of its predecessor (or C where there is none)
template <int VPL> __device__ inline void sgm_step(int* L, const int* C, bool restart, int d0, int size_d, int p1, int p2) {
    int nl[VPL];
    if (restart) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) nl[j] = d0 + j < size_d ? C[j] : SGM_BIG;
    } else {
        int lm = L[0];
#pragma unroll
        for (int j = 1; j < VPL; ++j) lm = min(lm, L[j]);
        const int m = wave_min(lm);
        const int below = from_lane_below(L[VPL - 1], SGM_BIG), above = from_lane_above(L[0], SGM_BIG);
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int lo = j > 0 ? L[j - 1] : below, hi = j < VPL - 1 ? L[j + 1] : above;
            const int t = min(min(L[j], min(lo, hi) + p1), m + p2) - m;
            nl[j] = d0 + j < size_d ? C[j] + t : SGM_BIG;
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) L[j] = nl[j];
}

// A walk over `len` pixels px(i) = the i-th pixel of the path.  STORE: S = L, else S += L.
template <int VPL, bool STORE, class PixelOf, class RestartAt>
__device__ inline void sgm_walk(const uint8_t* c8, uint16_t* s16, int len, int dp, int size_d, int p1, int p2, int lane,
                                PixelOf pixel_of, RestartAt restart_at) {
    typedef typename Pk<VPL>::C CT;
    typedef typename Pk<VPL>::S ST;
    const int d0 = lane * VPL;
    const bool on = d0 < dp;                  // lanes past the padded range touch no memory
    int L[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) L[j] = SGM_BIG;
    CT cw = CT();
    ST sw = ST();
    int64_t px = pixel_of(0);
    if (on) {
        cw = *reinterpret_cast<const CT*>(c8 + px * dp + d0);
        if (!STORE) sw = *reinterpret_cast<const ST*>(s16 + px * dp + d0);
    }
    for (int i = 0; i < len; ++i) {
        CT cn = CT();
        ST sn = ST();
        int64_t pn = px;
        if (i + 1 < len) {
            pn = pixel_of(i + 1);
            if (on) {
                cn = *reinterpret_cast<const CT*>(c8 + pn * dp + d0);
                if (!STORE) sn = *reinterpret_cast<const ST*>(s16 + pn * dp + d0);
            }
        }
        int C[VPL], S[VPL];
        unpack_c<VPL>(cw, C);
        sgm_step<VPL>(L, C, restart_at(i), d0, size_d, p1, p2);
        if (STORE) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) S[j] = 0;
        } else {
            unpack_s(sw, S);
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) S[j] += d0 + j < size_d ? L[j] : 0;
        if (on) {
            ST out;
            pack_s(S, &out);
            *reinterpret_cast<ST*>(s16 + px * dp + d0) = out;
        }
        cw = cn; sw = sn; px = pn;
    }
}

// grid (ceil(h / SGM_WAVES), nviews): a wave per row, (1, 0) then (-1, 0)
template <int VPL> __global__ __launch_bounds__(64 * SGM_WAVES) void k_sgm_rows(const SgmArgs a) {
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int y = (int)blockIdx.x * SGM_WAVES + (int)(threadIdx.x >> 6);
    if (y >= a.h) return;
    const int64_t row = (int64_t)y * a.w;
    const int w = a.w;
    sgm_walk<VPL, true>(a.c8[v], a.s16[v], w, a.dp, a.size_d, a.p1, a.p2, lane,
                        [=](int i) { return row + i; }, [](int i) { return i == 0; });
    sgm_walk<VPL, false>(a.c8[v], a.s16[v], w, a.dp, a.size_d, a.p1, a.p2, lane,
                         [=](int i) { return row + (w - 1 - i); }, [](int i) { return i == 0; });
}

// grid (ceil(w / SGM_WAVES), nviews): a wave per start column; direction (dx, dy), dy = +-1, dx in {-1, 0, 1}
template <int VPL> __global__ __launch_bounds__(64 * SGM_WAVES) void k_sgm_cols(const SgmArgs a, int dx, int dy) {
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int x0 = (int)blockIdx.x * SGM_WAVES + (int)(threadIdx.x >> 6);
    if (x0 >= a.w) return;
    const int w = a.w, h = a.h;
    // the column of step i: (x0 + dx * i) mod w; the predecessor of a pixel lies outside the image in the first row of the
    // walk and where the column has just wrapped (column 0 for dx = 1, column w - 1 for dx = -1)
    auto col = [=](int i) { const int s = i % w; int x = x0 + dx * s; x = x >= w ? x - w : x; return x < 0 ? x + w : x; };
    const int entry = dx > 0 ? 0 : w - 1;
    sgm_walk<VPL, false>(a.c8[v], a.s16[v], h, a.dp, a.size_d, a.p1, a.p2, lane,
                         [=](int i) { return (int64_t)(dy > 0 ? i : h - 1 - i) * w + col(i); },
                         [=](int i) { return i == 0 || (dx != 0 && col(i) == entry); });
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

template <int VPL> int launch_paths(const SgmArgs& a, int nviews, int paths, hipStream_t st) {
    const dim3 block(64 * SGM_WAVES);
    hipLaunchKernelGGL(k_sgm_rows<VPL>, dim3((unsigned)((a.h + SGM_WAVES - 1) / SGM_WAVES), (unsigned)nviews), block, 0, st, a);
    SMX_HIP(hipGetLastError());
    const dim3 grid((unsigned)((a.w + SGM_WAVES - 1) / SGM_WAVES), (unsigned)nviews);
    static const int dirs[6][2] = {{0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    for (int k = 0; k < paths - 2; ++k) {
        hipLaunchKernelGGL(k_sgm_cols<VPL>, grid, block, 0, st, a, dirs[k][0], dirs[k][1]);
        SMX_HIP(hipGetLastError());
    }
    return SMX_OK;
}

size_t sgm_plane_bytes(int w, int h, int size_d) { return align_up((size_t)w * h * (size_t)sgm_padded_d(size_d), 256); }

}  // namespace

int sgm_padded_d(int size_d) { return (size_d + 63) / 64 * 64; }

size_t sgm_workspace_bytes(int w, int h, int size_d, int nviews) {
    return 255 + (size_t)nviews * 3 * sgm_plane_bytes(w, h, size_d);       // per view: C8 (one plane) and S16 (two)
}

int launch_sgm_wta_pair(int p1, int p2, int paths, const float* cost_l, const float* cost_r, int w, int h, int size_d,
                        int64_t* keys, float* agg, float* nbr, float* uq, void* ws, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    SgmArgs a = {};
    const ViewSlots s = view_slots(cost_l, cost_r, keys, agg, nbr, uq, size_d, n);
    const int nviews = s.V;
    const float* costs[2] = {cost_l, cost_r};
    const size_t plane = sgm_plane_bytes(w, h, size_d);
    uint8_t* base = reinterpret_cast<uint8_t*>(align_up((size_t)ws, 256));
    s.put(a);
    for (int k = 0; k < nviews; ++k) {
        a.cost[k] = costs[s.view[k]];
        a.c8[k] = base + (size_t)k * 3 * plane;
        a.s16[k] = reinterpret_cast<uint16_t*>(base + (size_t)k * 3 * plane + plane);
    }
    a.w = w; a.h = h; a.size_d = size_d; a.dp = sgm_padded_d(size_d); a.p1 = p1; a.p2 = p2;
    a.xtiles = (w + SGM_TILE - 1) / SGM_TILE;
    const long long tiles = (long long)a.xtiles * h;
    if (tiles > 0x7FFFFFFFll) return fail(SMX_E_ARG, "smx_dev_sgm_wta_pair: %d x %d is too many tiles", w, h);
    hipLaunchKernelGGL(k_sgm_pack, dim3((unsigned)tiles, (unsigned)(a.dp / SGM_TILE), (unsigned)nviews), dim3(256), 0, st, a);
    SMX_HIP(hipGetLastError());
    int rc;
    if (a.dp == 64) rc = launch_paths<1>(a, nviews, paths, st);
    else if (a.dp == 128) rc = launch_paths<2>(a, nviews, paths, st);
    else rc = launch_paths<4>(a, nviews, paths, st);
    if (rc) return rc;
    const size_t lds = (size_t)SGM_TILE * (a.dp / 2 + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(k_sgm_select, dim3((unsigned)tiles, (unsigned)nviews), dim3(256), lds, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
