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
// k_sgm_pack, k_sgm_select and the register helpers of a step live in smx_sgm_dev.h: smx_scanline.hip builds on them too.
#include "smx_sgm_dev.h"

namespace smx {
namespace {

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
