// Hierarchical min-sum belief propagation on the 4-connected grid (Felzenszwalb and Huttenlocher, IJCV 2006) as an opt-in
// aggregation of a cost volume.  Not a stage of the reference.  Contract (clamp, pyramid, messages, schedule, tie rule,
// outputs): include/smx.h, above smx_bp_params.
//
// Layout.  As in smx_sgm.hip every plane of the workspace is [y][x][Dp] with Dp = size_d rounded up to 64, and lane l of a
// wave owns the VPL consecutive labels l * VPL .. (VPL = 1, 2, 4 for Dp = 64, 128, <= 256).  Per view and level l:
//   DATA  the data term: u8 at level 0 (k_bp_pack: smx_sgm_dev.h's pack with the data_scale product in front of the
//         clamp), u32 at the coarse levels (k_bp_coarse: the sum of the up to four children; D_l <= 255 * 4^l)
//   MSG   four u16 planes: the incoming messages of a pixel from its left, right, upper and lower neighbour (0 <= m <= trunc)
// and per view one u16 plane S16 with the belief of level 0, which smx_sgm_dev.h's k_sgm_select turns into keys, agg, nbr, uq.
//
// k_bp_iter: ONE WAVE PER SENDING PIXEL of the parity that is not being updated.  It loads the pixel's data term and its four
// incoming messages (one packed load each), forms tot = D + sum m, and for every direction with a neighbour takes
// h = tot - (the message from that neighbour), runs the min-convolution in registers and stores the message into the
// neighbour's slot.  Reads touch slots of the sender's parity only, writes slots of the other parity only: no hazard, no
// atomics, no LDS, no barrier.  The min-convolution with min(step |z - z'|, trunc) is two prefix minima over the labels,
//   m'(z) = min(step z + min_{z' <= z} (h(z') - step z'),  -step z + min_{z' >= z} (h(z') + step z'),  min h + trunc),
// each a serial pass over the lane's VPL labels, a log-step DPP scan inside every row of 16 lanes, three v_readlane for the
// rows before (after) the lane's own and one DPP wave shift to make the scan exclusive.  min_k m'(k) == min h (V(z, z) = 0),
// so one wave minimum normalises the message.  Labels >= size_d hold BP_BIG, which loses every minimum.
// k_bp_spread copies the parents' messages to the children, k_bp_belief writes S16.
#include "smx_sgm_dev.h"

namespace smx {
namespace {

constexpr int BP_BIG = 1 << 28;         // "no such label": above every h (<= 255 * 4^7 + 3 * 4095) plus step * z, far from overflow
constexpr int BP_WAVES = 4;             // sending pixels per workgroup of k_bp_iter
constexpr int BP_MAX_LEVELS = 8;

struct BpLevel {
    int w, h;
    void* data[2];          // u8 (level 0) or u32 (coarse) [y][x][dp]
    uint16_t* msg[2];       // [4][y][x][dp]
};

struct BpPackArgs {
    const float* cost[2];
    uint8_t* c8[2];
    int w, h, size_d, dp, xtiles;
    float scale;
};

// k_sgm_pack with t = c * scale in front of the clamp.  grid (xtiles * h, dp / 64, nviews), 256 threads
__global__ __launch_bounds__(256) void k_bp_pack(const BpPackArgs a) {
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
            if (d < a.size_d && x0 + x < a.w) c = clamp_cost(cost[(int64_t)d * n + row + x0 + x] * a.scale);
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

// the data term of a coarse level from the level below it (SRC: u8 at level 0, u32 above).  One thread per label of a coarse
// cell; grid (ceil(cw * ch * dp / 256), nviews), 256 threads
template <class SRC> __global__ __launch_bounds__(256) void k_bp_coarse(const BpLevel fine, const BpLevel coarse, int dp) {
    const int v = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cell = e / dp;
    if (cell >= (int64_t)coarse.w * coarse.h) return;
    const int d = (int)(e - cell * dp);
    const int cy = (int)(cell / coarse.w), cx = (int)(cell - (int64_t)cy * coarse.w);
    const SRC* src = static_cast<const SRC*>(fine.data[v]);
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int x = 2 * cx + i, y = 2 * cy + j;
            if (x < fine.w && y < fine.h) sum += src[((int64_t)y * fine.w + x) * dp + d];
        }
    }
    static_cast<uint32_t*>(coarse.data[v])[e] = sum;
}

// the messages of a level from its parents: cell (x, y) takes all four of (x >> 1, y >> 1).  One thread per 8 bytes (four
// labels); grid (ceil(w * h * dp / 4 / 256), 4, nviews), 256 threads
__global__ __launch_bounds__(256) void k_bp_spread(const BpLevel coarse, const BpLevel fine, int dp) {
    const int v = blockIdx.z, q = dp / 4;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t cell = e / q, cells = (int64_t)fine.w * fine.h;
    if (cell >= cells) return;
    const int k = (int)(e - cell * q);
    const int y = (int)(cell / fine.w), x = (int)(cell - (int64_t)y * fine.w);
    const int64_t parent = (int64_t)(y >> 1) * coarse.w + (x >> 1);
    const uint2* src = reinterpret_cast<const uint2*>(coarse.msg[v]) + (int64_t)blockIdx.y * coarse.w * coarse.h * q;
    uint2* dst = reinterpret_cast<uint2*>(fine.msg[v]) + (int64_t)blockIdx.y * cells * q;
    dst[e] = src[parent * q + k];
}

// all messages of a level = 0.  One thread per 8 bytes; grid (ceil(4 * w * h * dp / 4 / 256), nviews)
__global__ __launch_bounds__(256) void k_bp_zero(const BpLevel lv, int dp) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)lv.w * lv.h * dp) return;           // 4 planes * (dp / 4) units a cell
    reinterpret_cast<uint2*>(lv.msg[blockIdx.y])[e] = make_uint2(0u, 0u);
}

// S16 = D_0 + the four messages of level 0.  One thread per label; grid (ceil(w * h * dp / 256), nviews)
__global__ __launch_bounds__(256) void k_bp_belief(const BpLevel lv, uint16_t* s16_l, uint16_t* s16_r, int dp) {
    const int v = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, plane = (int64_t)lv.w * lv.h * dp;
    if (e >= plane) return;
    const uint16_t* m = lv.msg[v];
    const uint32_t s = static_cast<const uint8_t*>(lv.data[v])[e] + (uint32_t)m[e] + m[plane + e] + m[2 * plane + e] + m[3 * plane + e];
    (v ? s16_r : s16_l)[e] = (uint16_t)s;
}

// ---- a message, all in registers --------------------------------------------------------------------------------------
__device__ inline int dpp_row_shr(int x, int n) {
    switch (n) {        // lane i <- lane i - n of its row of 16, BP_BIG where there is none
    case 1: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x111, 0xF, 0xF, false);
    case 2: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x112, 0xF, 0xF, false);
    case 4: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x114, 0xF, 0xF, false);
    default: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x118, 0xF, 0xF, false);
    }
}
__device__ inline int dpp_row_shl(int x, int n) {
    switch (n) {        // lane i <- lane i + n of its row of 16, BP_BIG where there is none
    case 1: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x101, 0xF, 0xF, false);
    case 2: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x102, 0xF, 0xF, false);
    case 4: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x104, 0xF, 0xF, false);
    default: return __builtin_amdgcn_update_dpp(BP_BIG, x, 0x108, 0xF, 0xF, false);
    }
}
// the minimum of x over the lanes BELOW this one (BP_BIG in lane 0); row = lane >> 4
__device__ inline int min_of_lanes_below(int x, int row) {
    x = min(x, dpp_row_shr(x, 1));
    x = min(x, dpp_row_shr(x, 2));
    x = min(x, dpp_row_shr(x, 4));
    x = min(x, dpp_row_shr(x, 8));
    const int r0 = __builtin_amdgcn_readlane(x, 15), r1 = __builtin_amdgcn_readlane(x, 31), r2 = __builtin_amdgcn_readlane(x, 47);
    const int r01 = min(r0, r1);
    x = min(x, row == 0 ? BP_BIG : row == 1 ? r0 : row == 2 ? r01 : min(r01, r2));
    return from_lane_below(x, BP_BIG);
}
// ... over the lanes ABOVE this one (BP_BIG in lane 63)
__device__ inline int min_of_lanes_above(int x, int row) {
    x = min(x, dpp_row_shl(x, 1));
    x = min(x, dpp_row_shl(x, 2));
    x = min(x, dpp_row_shl(x, 4));
    x = min(x, dpp_row_shl(x, 8));
    const int r1 = __builtin_amdgcn_readlane(x, 16), r2 = __builtin_amdgcn_readlane(x, 32), r3 = __builtin_amdgcn_readlane(x, 48);
    const int r23 = min(r2, r3);
    x = min(x, row == 3 ? BP_BIG : row == 2 ? r3 : row == 1 ? r23 : min(r23, r1));
    return from_lane_above(x, BP_BIG);
}

// out = the normalised message of h (BP_BIG at labels >= size_d; out is 0 there).  d0: the lane's first label
template <int VPL> __device__ inline void bp_message(const int* h, int* out, int d0, int size_d, int step, int trunc, int row) {
    int lm = h[0];
#pragma unroll
    for (int j = 1; j < VPL; ++j) lm = min(lm, h[j]);
    const int mh = wave_min(lm);
    int up[VPL], dn[VPL];
    int run = BP_BIG;
#pragma unroll
    for (int j = 0; j < VPL; ++j) { run = min(run, h[j] - step * (d0 + j)); up[j] = run; }
    const int below = min_of_lanes_below(run, row);
    run = BP_BIG;
#pragma unroll
    for (int j = VPL - 1; j >= 0; --j) { run = min(run, h[j] + step * (d0 + j)); dn[j] = run; }
    const int above = min_of_lanes_above(run, row);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int z = d0 + j;
        const int m = min(min(min(up[j], below) + step * z, min(dn[j], above) - step * z), mh + trunc) - mh;
        out[j] = z < size_d ? m : 0;
    }
}

template <int VPL> struct BpData;        // the VPL u32 data terms of a lane at a coarse level as one load
template <> struct BpData<1> { typedef uint32_t T; };
template <> struct BpData<2> { typedef uint2 T; };
template <> struct BpData<4> { typedef uint4 T; };
__device__ inline void unpack_d(uint32_t d, int* out) { out[0] = (int)d; }
__device__ inline void unpack_d(uint2 d, int* out) { out[0] = (int)d.x; out[1] = (int)d.y; }
__device__ inline void unpack_d(uint4 d, int* out) { out[0] = (int)d.x; out[1] = (int)d.y; out[2] = (int)d.z; out[3] = (int)d.w; }

// Iteration t of a level: the pixels with (x + y + t) odd send.  grid (ceil(ceil(w / 2) / BP_WAVES) * h, nviews)
template <int VPL, bool COARSE> __global__ __launch_bounds__(64 * BP_WAVES) void k_bp_iter(const BpLevel lv, int dp, int size_d,
                                                                                            int step, int trunc, int t, int xblocks) {
    typedef typename Pk<VPL>::S ST;
    const int v = blockIdx.y, lane = threadIdx.x & 63;
    const int y = (int)(blockIdx.x / (unsigned)xblocks);
    const int i = (int)(blockIdx.x % (unsigned)xblocks) * BP_WAVES + (int)(threadIdx.x >> 6);
    const int x = 2 * i + ((y + t + 1) & 1);
    if (x >= lv.w) return;                    // (the whole wave)
    const int w = lv.w, h = lv.h;
    const int d0 = lane * VPL, row = lane >> 4;
    const bool on = d0 < dp;                  // lanes past the padded range touch no memory
    const int64_t cells = (int64_t)w * h, px = (int64_t)y * w + x, at = px * dp + d0;
    uint16_t* msg = lv.msg[v];
    int D[VPL], m[4][VPL], tot[VPL];
#pragma unroll
    for (int j = 0; j < VPL; ++j) D[j] = 0;
    ST mw[4] = {ST(), ST(), ST(), ST()};
    if (on) {
        if (COARSE) {
            unpack_d(*reinterpret_cast<const typename BpData<VPL>::T*>(static_cast<const uint32_t*>(lv.data[v]) + at), D);
        } else {
            unpack_c<VPL>(*reinterpret_cast<const typename Pk<VPL>::C*>(static_cast<const uint8_t*>(lv.data[v]) + at), D);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) mw[k] = *reinterpret_cast<const ST*>(msg + k * cells * dp + at);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) unpack_s(mw[k], m[k]);
#pragma unroll
    for (int j = 0; j < VPL; ++j) tot[j] = D[j] + m[0][j] + m[1][j] + m[2][j] + m[3][j];
    // towards the neighbour in direction k' the pixel leaves out what came from there (slot k') and writes the neighbour's
    // slot of the opposite direction: 0 <-> 1 (left, right), 2 <-> 3 (up, down)
    const bool has[4] = {x > 0, x + 1 < w, y > 0, y + 1 < h};
    const int64_t nb[4] = {px - 1, px + 1, px - w, px + w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!has[k]) continue;                // (uniform over the wave)
        int hv[VPL], out[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) hv[j] = d0 + j < size_d ? tot[j] - m[k][j] : BP_BIG;
        bp_message<VPL>(hv, out, d0, size_d, step, trunc, row);
        if (on) {
            ST o;
            pack_s(out, &o);
            *reinterpret_cast<ST*>(msg + (k ^ 1) * cells * dp + nb[k] * dp + d0) = o;
        }
    }
}

inline void level_size(int w, int h, int l, int* lw, int* lh) {
    for (; l > 0; --l) { w = (w + 1) / 2; h = (h + 1) / 2; }
    *lw = w; *lh = h;
}
inline size_t bp_data_bytes(int lw, int lh, int dp, int l) { return align_up((size_t)(l ? 4 : 1) * lw * lh * dp, 256); }
inline size_t bp_msg_bytes(int lw, int lh, int dp) { return align_up((size_t)8 * lw * lh * dp, 256); }

template <int VPL> int launch_iterations(const BpLevel& lv, bool coarse, int nviews, int dp, int size_d, const smx_bp_params* p,
                                         hipStream_t st) {
    const int xblocks = ((lv.w + 1) / 2 + BP_WAVES - 1) / BP_WAVES;
    const dim3 grid((unsigned)((long long)xblocks * lv.h), (unsigned)nviews), block(64 * BP_WAVES);
    for (int t = 1; t <= p->iterations; ++t) {
        if (coarse) hipLaunchKernelGGL((k_bp_iter<VPL, true>), grid, block, 0, st, lv, dp, size_d, p->step, p->trunc, t, xblocks);
        else hipLaunchKernelGGL((k_bp_iter<VPL, false>), grid, block, 0, st, lv, dp, size_d, p->step, p->trunc, t, xblocks);
        SMX_HIP(hipGetLastError());
    }
    return SMX_OK;
}

}  // namespace

size_t bp_workspace_bytes(int w, int h, int size_d, int levels, int nviews) {
    const int dp = sgm_padded_d(size_d);
    size_t view = align_up((size_t)2 * w * h * dp, 256);          // S16
    for (int l = 0; l < levels; ++l) {
        int lw, lh;
        level_size(w, h, l, &lw, &lh);
        view += bp_data_bytes(lw, lh, dp, l) + bp_msg_bytes(lw, lh, dp);
    }
    return 255 + (size_t)nviews * view;
}

int launch_bp_wta_pair(const smx_bp_params* p, const float* cost_l, const float* cost_r, int w, int h, int size_d, int64_t* keys,
                       float* agg, float* nbr, float* uq, void* ws, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    const int dp = sgm_padded_d(size_d), levels = p->levels;
    const ViewSlots s = view_slots(cost_l, cost_r, keys, agg, nbr, uq, size_d, n);
    const int nviews = s.V;
    const float* costs[2] = {cost_l, cost_r};
    const int xtiles = (w + SGM_TILE - 1) / SGM_TILE;
    const long long tiles = (long long)xtiles * h;
    if (tiles > 0x7FFFFFFFll || ((long long)(w + 1) / 2 + BP_WAVES - 1) / BP_WAVES * h > 0x7FFFFFFFll)
        return fail(SMX_E_ARG, "smx_dev_bp_wta_pair: %d x %d is too many tiles", w, h);
    // the workspace: per view S16, then DATA and MSG of every level
    BpLevel lv[BP_MAX_LEVELS] = {};
    SgmArgs sel = {};
    s.put(sel);
    uint8_t* at = reinterpret_cast<uint8_t*>(align_up((size_t)ws, 256));
    for (int l = 0; l < levels; ++l) level_size(w, h, l, &lv[l].w, &lv[l].h);
    for (int k = 0; k < nviews; ++k) {
        sel.s16[k] = reinterpret_cast<uint16_t*>(at);
        at += align_up((size_t)2 * n * dp, 256);
        for (int l = 0; l < levels; ++l) {
            lv[l].data[k] = at;
            at += bp_data_bytes(lv[l].w, lv[l].h, dp, l);
            lv[l].msg[k] = reinterpret_cast<uint16_t*>(at);
            at += bp_msg_bytes(lv[l].w, lv[l].h, dp);
        }
    }
    sel.w = w; sel.h = h; sel.size_d = size_d; sel.dp = dp; sel.xtiles = xtiles;
    BpPackArgs pk = {};
    for (int k = 0; k < nviews; ++k) {
        pk.cost[k] = costs[s.view[k]];
        pk.c8[k] = static_cast<uint8_t*>(lv[0].data[k]);
    }
    pk.w = w; pk.h = h; pk.size_d = size_d; pk.dp = dp; pk.xtiles = xtiles; pk.scale = p->data_scale;
    hipLaunchKernelGGL(k_bp_pack, dim3((unsigned)tiles, (unsigned)(dp / SGM_TILE), (unsigned)nviews), dim3(256), 0, st, pk);
    SMX_HIP(hipGetLastError());
    auto blocks = [](long long units) { return (unsigned)((units + 255) / 256); };
    for (int l = 1; l < levels; ++l) {
        const dim3 grid(blocks((long long)lv[l].w * lv[l].h * dp), (unsigned)nviews);
        if (l == 1) hipLaunchKernelGGL(k_bp_coarse<uint8_t>, grid, dim3(256), 0, st, lv[0], lv[1], dp);
        else hipLaunchKernelGGL(k_bp_coarse<uint32_t>, grid, dim3(256), 0, st, lv[l - 1], lv[l], dp);
        SMX_HIP(hipGetLastError());
    }
    {
        const BpLevel& top = lv[levels - 1];
        hipLaunchKernelGGL(k_bp_zero, dim3(blocks((long long)top.w * top.h * dp), (unsigned)nviews), dim3(256), 0, st, top, dp);
        SMX_HIP(hipGetLastError());
    }
    for (int l = levels - 1; l >= 0; --l) {
        if (l < levels - 1) {
            hipLaunchKernelGGL(k_bp_spread, dim3(blocks((long long)lv[l].w * lv[l].h * (dp / 4)), 4u, (unsigned)nviews), dim3(256), 0,
                               st, lv[l + 1], lv[l], dp);
            SMX_HIP(hipGetLastError());
        }
        int rc;
        if (dp == 64) rc = launch_iterations<1>(lv[l], l > 0, nviews, dp, size_d, p, st);
        else if (dp == 128) rc = launch_iterations<2>(lv[l], l > 0, nviews, dp, size_d, p, st);
        else rc = launch_iterations<4>(lv[l], l > 0, nviews, dp, size_d, p, st);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_bp_belief, dim3(blocks((long long)n * dp), (unsigned)nviews), dim3(256), 0, st, lv[0], sel.s16[0], sel.s16[1],
                       dp);
    SMX_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_sgm_select, dim3((unsigned)tiles, (unsigned)nviews), dim3(256), sgm_select_lds(dp), st, sel);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
