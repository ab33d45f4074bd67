// Scan-line optimisation with colour-adaptive penalties (Mei et al. 2011, the step between the cross-based aggregation and the
// winners).  Not a stage of the reference.  Contract (flags, penalties, recurrence, outputs): include/smx.h,
// smx_dev_scanline_wta_pair.  It is the recurrence of smx_sgm.hip with penalties that depend on the pixel, the direction and
// the label, and it is built on that file's scheme: the planes C8 and S16 [y][x][Dp], k_sgm_pack in front and k_sgm_select
// behind (smx_sgm_dev.h), one wave per path with all labels of the path's pixel in registers.
//
// k_so_edges: one launch writes, for each view, a u8 plane E [y][SO_PAD + x + SO_PAD] whose bit i says that the colour step
//   from p - DIRS8[i] to p is an edge, D(p, p - r) >= tau_so, and is 0 where p - r lies outside the image.  The SO_PAD bytes
//   at both ends of a row are written as 0.  A label's partner q = (x + d, y) lies in the same row of the OTHER view's plane,
//   so both flags of a step are bits of these planes: e1 = E_own[y][x], e2 = E_other[y][x + d], and "q or q - r outside the
//   image" needs no test of its own: a partner column clamped to [-SO_PAD, w] reads a padding byte, and a partner whose
//   predecessor is outside has the bit 0.  Both planes are always built: a view's e2 reads the other one.
// k_so_rows / k_so_cols: the walks of k_sgm_rows / k_sgm_cols.  New per step: the own byte (one address for the whole wave,
//   made scalar by v_readfirstlane, so the choice between the penalty pairs of k and k + 1 is scalar) and the VPL partner
//   bytes of the lane as ONE unaligned load of VPL bytes from the padded row; then one v_cndmask per label and penalty.
//   Both loads are issued with the next pixel's C and S, one step ahead of their use, and stay off the dependent chain.
#include "smx_sgm_dev.h"

namespace smx {
namespace {

constexpr int SO_PAD = 4;               // zero bytes at both ends of an edge row: the widest partner load is 4 bytes

struct SoArgs {
    SgmArgs s;               // the planes and outputs of the views of this launch; p1, p2 unused
    const uint8_t* guide[2]; // by the caller's view (0 left, 1 right): always both
    uint8_t* edge[2];        // by the caller's view: [h][es]
    int view[2];             // view k of the launch is the caller's view[k]
    int dmin[2];             // by the caller's view
    int64_t es;              // bytes of an edge row: w + 2 * SO_PAD
    int channels, nch, tau;  // nch = min(channels, 3): the channels D looks at
    int p1k[3], p2k[3];      // the penalties of k = e1 + e2 = 0, 1, 2
};

// grid (ceil(es / 256), min(h, 65535), 2), 256 threads: a thread per byte of a row, rows in a grid-stride loop
__global__ __launch_bounds__(256) void k_so_edges(const SoArgs a) {
    const int v = blockIdx.z;
    const int64_t xp = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (xp >= a.es) return;
    const int w = a.s.w, h = a.s.h, ch = a.channels, nch = a.nch;
    const int64_t x = xp - SO_PAD;
    const uint8_t* g = a.guide[v];
    const int dxs[8] = {1, -1, 0, 0, 1, -1, 1, -1}, dys[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    for (int y = blockIdx.y; y < h; y += gridDim.y) {
        unsigned bits = 0;
        if (x >= 0 && x < w) {
            const uint8_t* p = g + ((int64_t)y * w + x) * ch;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int64_t qx = x - dxs[i];
                const int qy = y - dys[i];
                if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                const uint8_t* q = g + ((int64_t)qy * w + qx) * ch;
                int d = 0;
                for (int c = 0; c < nch; ++c) d = max(d, abs((int)p[c] - (int)q[c]));
                bits |= (d >= a.tau ? 1u : 0u) << i;
            }
        }
        a.edge[v][(int64_t)y * a.es + xp] = (uint8_t)bits;
    }
}

// the VPL partner bytes of a lane, byte j in bits 8j ..: one load, of any alignment
template <int VPL> __device__ inline uint32_t load_flags(const uint8_t* p);
template <> __device__ inline uint32_t load_flags<1>(const uint8_t* p) { return *p; }
template <> __device__ inline uint32_t load_flags<2>(const uint8_t* p) {
    struct __attribute__((packed)) U { uint16_t v; };
    return reinterpret_cast<const U*>(p)->v;
}
template <> __device__ inline uint32_t load_flags<4>(const uint8_t* p) {
    struct __attribute__((packed)) U { uint32_t v; };
    return reinterpret_cast<const U*>(p)->v;
}

struct SoPen { int p1k[3], p2k[3]; };

// L <- the path costs of the next pixel from those of its predecessor (or C where there is none).  own: the pixel's own flag
// (scalar), part: the partner bytes of the lane's labels, bit: the direction's bit in them.
template <int VPL>
__device__ inline void so_step(int* L, const int* C, bool restart, int d0, int size_d, const SoPen& pen, int own, uint32_t part,
                               int bit) {
    int nl[VPL];
    if (restart) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) nl[j] = d0 + j < size_d ? C[j] : SGM_BIG;
    } else {
        // k = own + e2: the pair of e2 = 0 and the pair of e2 = 1, both scalar
        const int p1lo = own ? pen.p1k[1] : pen.p1k[0], p1hi = own ? pen.p1k[2] : pen.p1k[1];
        const int p2lo = own ? pen.p2k[1] : pen.p2k[0], p2hi = own ? pen.p2k[2] : pen.p2k[1];
        int lm = L[0];
#pragma unroll
        for (int j = 1; j < VPL; ++j) lm = min(lm, L[j]);
        const int m = wave_min(lm);
        const int below = from_lane_below(L[VPL - 1], SGM_BIG), above = from_lane_above(L[0], SGM_BIG);
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const bool e2 = ((part >> (8 * j + bit)) & 1u) != 0;
            const int p1 = e2 ? p1hi : p1lo, p2 = e2 ? p2hi : p2lo;
            const int lo = j > 0 ? L[j - 1] : below, hi = j < VPL - 1 ? L[j + 1] : above;
            const int t = min(min(L[j], min(lo, hi) + p1), m + p2) - m;
            nl[j] = d0 + j < size_d ? C[j] + t : SGM_BIG;
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) L[j] = nl[j];
}

struct SoWalk {
    const uint8_t* c8;
    uint16_t* s16;
    const uint8_t* eown;     // the view's own edge plane, at column 0 of row 0
    const uint8_t* eoth;     // the other view's
    int64_t es;
    int w, dp, size_d, dmin, bit;
    SoPen pen;
};

// A walk over `len` pixels; xy_of(i) = the i-th pixel of the path as (x, y).  STORE: S = L, else S += L.
template <int VPL, bool STORE, class XyOf, class RestartAt>
__device__ inline void so_walk(const SoWalk& k, int len, int lane, XyOf xy_of, RestartAt restart_at) {
    typedef typename Pk<VPL>::C CT;
    typedef typename Pk<VPL>::S ST;
    const int d0 = lane * VPL, dp = k.dp;
    const bool on = d0 < dp;                  // lanes past the padded range touch no memory
    const int64_t off = (int64_t)k.dmin + d0; // the partner column of the lane's first label is x + off
    const int64_t xhi = k.w;
    int L[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) L[j] = SGM_BIG;
    CT cw = CT();
    ST sw = ST();
    uint32_t ow = 0, fw = 0;
    // the loads of a pixel: costs, sums, the own byte and the partner bytes; a partner column left of -SO_PAD or right of w
    // reads the row's padding, which holds 0
    auto fetch = [&](int x, int y, CT& c, ST& s, uint32_t& o, uint32_t& f) {
        const int64_t px = (int64_t)y * k.w + x;
        const int64_t erow = (int64_t)y * k.es;
        int64_t xq = x + off;
        xq = xq < -SO_PAD ? -SO_PAD : (xq > xhi ? xhi : xq);
        if (on) {
            o = k.eown[erow + x];
            c = *reinterpret_cast<const CT*>(k.c8 + px * dp + d0);
            if (!STORE) s = *reinterpret_cast<const ST*>(k.s16 + px * dp + d0);
            f = load_flags<VPL>(k.eoth + erow + xq);
        }
        return px;
    };
    int2 xy = xy_of(0);
    int64_t px = fetch(xy.x, xy.y, cw, sw, ow, fw);
    for (int i = 0; i < len; ++i) {
        CT cn = CT();
        ST sn = ST();
        uint32_t on_ = 0, fn = 0;
        int64_t pn = px;
        if (i + 1 < len) {
            xy = xy_of(i + 1);
            pn = fetch(xy.x, xy.y, cn, sn, on_, fn);
        }
        int C[VPL], S[VPL];
        unpack_c<VPL>(cw, C);
        const int own = (__builtin_amdgcn_readfirstlane((int)ow) >> k.bit) & 1;
        so_step<VPL>(L, C, restart_at(i), d0, k.size_d, k.pen, own, fw, k.bit);
        if (STORE) {
#pragma unroll
            for (int j = 0; j < VPL; ++j) S[j] = 0;
        } else {
            unpack_s(sw, S);
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) S[j] += d0 + j < k.size_d ? L[j] : 0;
        if (on) {
            ST out;
            pack_s(S, &out);
            *reinterpret_cast<ST*>(k.s16 + px * dp + d0) = out;
        }
        // The prefetch is taken over here, behind the step's arithmetic and its store: s_waitcnt vmcnt(1) with the other counters
        // open, fenced against the scheduler.  Left to itself the compiler puts its own vmcnt(0) right behind the loads' issue in
        // some instantiations (it did in k_so_rows<2>, and in all of them before the wave's number was made scalar), and then
        // every step pays the latency of its loads.
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0F71);
        __builtin_amdgcn_sched_barrier(0);
        cw = cn; sw = sn; ow = on_; fw = fn; px = pn;
    }
}

__device__ inline SoWalk so_walk_of(const SoArgs& a, int v, int bit) {
    const int own = a.view[v];
    SoWalk k;
    k.c8 = a.s.c8[v]; k.s16 = a.s.s16[v];
    k.eown = a.edge[own] + SO_PAD; k.eoth = a.edge[1 - own] + SO_PAD;
    k.es = a.es; k.w = a.s.w; k.dp = a.s.dp; k.size_d = a.s.size_d; k.dmin = a.dmin[own]; k.bit = bit;
    for (int i = 0; i < 3; ++i) { k.pen.p1k[i] = a.p1k[i]; k.pen.p2k[i] = a.p2k[i]; }
    return k;
}

// grid (ceil(h / SGM_WAVES), nviews): a wave per row, (1, 0) then (-1, 0): bits 0 and 1
template <int VPL> __global__ __launch_bounds__(64 * SGM_WAVES) void k_so_rows(const SoArgs a) {
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    // (the wave's number made scalar: a step's addresses are a scalar base and a lane offset that never changes)
    const int y = (int)blockIdx.x * SGM_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (y >= a.s.h) return;
    const int w = a.s.w;
    so_walk<VPL, true>(so_walk_of(a, v, 0), w, lane, [=](int i) { return make_int2(i, y); }, [](int i) { return i == 0; });
    so_walk<VPL, false>(so_walk_of(a, v, 1), w, lane, [=](int i) { return make_int2(w - 1 - i, y); },
                        [](int i) { return i == 0; });
}

// grid (ceil(w / SGM_WAVES), nviews): a wave per start column; direction (dx, dy) = DIRS8[bit], dy = +-1, dx in {-1, 0, 1}
template <int VPL> __global__ __launch_bounds__(64 * SGM_WAVES) void k_so_cols(const SoArgs a, int dx, int dy, int bit) {
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int x0 = (int)blockIdx.x * SGM_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (x0 >= a.s.w) return;
    const int w = a.s.w, h = a.s.h;
    // the column of step i and the restarts: as in k_sgm_cols
    auto col = [=](int i) { const int s = i % w; int x = x0 + dx * s; x = x >= w ? x - w : x; return x < 0 ? x + w : x; };
    const int entry = dx > 0 ? 0 : w - 1;
    so_walk<VPL, false>(so_walk_of(a, v, bit), h, lane, [=](int i) { return make_int2(col(i), dy > 0 ? i : h - 1 - i); },
                        [=](int i) { return i == 0 || (dx != 0 && col(i) == entry); });
}

template <int VPL> int launch_so_paths(const SoArgs& a, int nviews, int paths, hipStream_t st) {
    const dim3 block(64 * SGM_WAVES);
    hipLaunchKernelGGL(k_so_rows<VPL>, dim3((unsigned)((a.s.h + SGM_WAVES - 1) / SGM_WAVES), (unsigned)nviews), block, 0, st, a);
    SMX_HIP(hipGetLastError());
    const dim3 grid((unsigned)((a.s.w + SGM_WAVES - 1) / SGM_WAVES), (unsigned)nviews);
    static const int dirs[6][2] = {{0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};      // DIRS8[2 ..]
    for (int k = 0; k < paths - 2; ++k) {
        hipLaunchKernelGGL(k_so_cols<VPL>, grid, block, 0, st, a, dirs[k][0], dirs[k][1], 2 + k);
        SMX_HIP(hipGetLastError());
    }
    return SMX_OK;
}

size_t so_edge_bytes(int w, int h) { return align_up((size_t)h * ((size_t)w + 2 * SO_PAD), 256); }

}  // namespace

size_t scanline_workspace_bytes(int w, int h, int size_d, int nviews) {
    return sgm_workspace_bytes(w, h, size_d, nviews) + 2 * so_edge_bytes(w, h);      // the SGM planes, then both edge planes
}

int launch_scanline_wta_pair(const smx_scanline_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch,
                             const float* cost_l, const float* cost_r, int w, int h, int size_d, int dminl, int dminr,
                             int64_t* keys, float* agg, float* nbr, float* uq, void* ws, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    SoArgs a = {};
    const ViewSlots s = view_slots(cost_l, cost_r, keys, agg, nbr, uq, size_d, n);
    const int nviews = s.V;
    const float* costs[2] = {cost_l, cost_r};
    const size_t plane = sgm_plane_bytes(w, h, size_d);
    uint8_t* base = reinterpret_cast<uint8_t*>(align_up((size_t)ws, 256));
    s.put(a.s);
    for (int k = 0; k < nviews; ++k) {
        a.s.cost[k] = costs[s.view[k]];
        a.s.c8[k] = base + (size_t)k * 3 * plane;
        a.s.s16[k] = reinterpret_cast<uint16_t*>(base + (size_t)k * 3 * plane + plane);
        a.view[k] = s.view[k];
    }
    uint8_t* edges = base + (size_t)nviews * 3 * plane;
    a.edge[0] = edges; a.edge[1] = edges + so_edge_bytes(w, h);
    a.guide[0] = guide_l; a.guide[1] = guide_r;
    a.dmin[0] = dminl; a.dmin[1] = dminr;
    a.es = (int64_t)w + 2 * SO_PAD;
    a.channels = ch; a.nch = ch < 3 ? ch : 3; a.tau = p->tau_so;
    const int div[3] = {1, 4, 10};
    for (int k = 0; k < 3; ++k) { a.p1k[k] = p->p1 / div[k]; a.p2k[k] = p->p2 / div[k]; }
    a.s.w = w; a.s.h = h; a.s.size_d = size_d; a.s.dp = sgm_padded_d(size_d);
    a.s.xtiles = (w + SGM_TILE - 1) / SGM_TILE;
    const long long tiles = (long long)a.s.xtiles * h;
    if (tiles > 0x7FFFFFFFll) return fail(SMX_E_ARG, "smx_dev_scanline_wta_pair: %d x %d is too many tiles", w, h);
    hipLaunchKernelGGL(k_so_edges, dim3((unsigned)((a.es + 255) / 256), (unsigned)(h < 65535 ? h : 65535), 2u), dim3(256), 0, st, a);
    SMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sgm_pack, dim3((unsigned)tiles, (unsigned)(a.s.dp / SGM_TILE), (unsigned)nviews), dim3(256), 0, st, a.s);
    SMX_HIP(hipGetLastError());
    int rc;
    if (a.s.dp == 64) rc = launch_so_paths<1>(a, nviews, p->paths, st);
    else if (a.s.dp == 128) rc = launch_so_paths<2>(a, nviews, p->paths, st);
    else rc = launch_so_paths<4>(a, nviews, p->paths, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sgm_select, dim3((unsigned)tiles, (unsigned)nviews), dim3(256), sgm_select_lds(a.s.dp), st, a.s);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
