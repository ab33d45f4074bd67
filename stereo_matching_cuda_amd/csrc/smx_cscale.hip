// smx_cscale.hip -- cross-scale cost aggregation (Zhang et al., CVPR 2014; not a stage of the reference: opt-in).  The definition
// is the comment above smx_cscale_params in include/smx.h and tests/cscale_ref.py, bit for bit: integers in the pyramid, and in
// the combination one f32 product per level and f32 sums in the order of the levels.
//
//   k_pyr_down    one level of the u8 pyramid: taps 1 4 6 4 1 in both directions on integers, reflect-101 borders, one output
//                 pixel per thread with all its channels, 64 x 4 outputs a workgroup.  25 byte loads per channel out of lines
//                 that the neighbouring lanes share; the images are small beside the volumes.
//   k_cscale      the combination and the winner-take-all pass over it, up to two views per launch (grid y).  Slices in natural
//                 order [z][h][w]; a lane owns EPL consecutive pixels (16-, 8- or 4-byte loads and stores of level 0 and
//                 out, nontemporal, four slices in flight) and loops over the slices ascending.  A value of level s serves 2^s
//                 labels of 2^s x 2^s pixels: its product with the level's weight stays in a register and is loaded again only
//                 where the label's ancestor changes ((dmin + z) a multiple of 2^s; uniform over the grid), once for the
//                 pixels of a lane that share it, and ahead of the slices that need it.  The winner state is WtaPixel
//                 (smx_wta.h), used as wta_launch's kernel uses it.  The optional store of the combined slice may go over the
//                 level-0 slice it came from: a lane reads exactly the elements it writes, and reads them first.
//                 No LDS, no barrier, no atomics, no division in the slice loop.
//
// Must be compiled with -ffp-contract=off.
#include "smx_api.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int PYR_TW = 64;      // output columns of a workgroup = lanes of a wave
constexpr int PYR_TH = 4;       // output rows of a workgroup = its waves

// reflect-101, then clamped: what is left to clamp only where N is 1 or 2
__device__ inline int reflect101(int i, int N) {
    i = i < 0 ? -i : i;
    i = i >= N ? 2 * (N - 1) - i : i;
    return i < 0 ? 0 : i > N - 1 ? N - 1 : i;
}

// grid: workgroup footprints of the output in row-major order.  src [h][w][CH], dst [(h+1)/2][(w+1)/2][CH]
template <int CH>
__global__ __launch_bounds__(PYR_TW * PYR_TH) void k_pyr_down(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int w,
                                                              int h) {
    const int wo = (w + 1) / 2, ho = (h + 1) / 2;
    const int tiles_x = (wo - 1) / PYR_TW + 1;
    const int xo = (int)(blockIdx.x % (unsigned)tiles_x) * PYR_TW + (int)(threadIdx.x & 63u);
    const int yo = (int)(blockIdx.x / (unsigned)tiles_x) * PYR_TH + (int)(threadIdx.x >> 6);
    if (xo >= wo || yo >= ho) return;
    const int tap[5] = {1, 4, 6, 4, 1};
    int xs[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) xs[i] = reflect101(2 * xo - 2 + i, w);
    int t[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) t[c] = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint8_t* row = src + (size_t)reflect101(2 * yo - 2 + j, h) * w * CH;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            int r = 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) r += tap[i] * (int)row[(size_t)xs[i] * CH + c];
            t[c] += tap[j] * r;
        }
    }
    uint8_t* o = dst + ((size_t)yo * wo + xo) * CH;
#pragma unroll
    for (int c = 0; c < CH; ++c) o[c] = (uint8_t)((t[c] + 128) >> 8);
}

constexpr int CS_TH = 2;        // rows of a workgroup of the combination
constexpr int CS_WX = 2;        // waves side by side in a row of it

struct CsArgs {
    const float* a[2][SMX_CSCALE_MAX_SCALES];       // per view: the levels' volumes
    float* out[2];                                  // NULL: the combined volume is not stored
    int64_t* keys[2];
    float *nbr[2], *uq[2];
    float wt[SMX_CSCALE_MAX_SCALES];
    int ws[SMX_CSCALE_MAX_SCALES], hs[SMX_CSCALE_MAX_SCALES];
    int dmin[2];
    int w, h, size_d, scales;
};

// grid (workgroup footprints in row-major order, views).  A workgroup takes CS_TH rows of CS_WX 64 EPL columns, a wave 64 EPL
// columns of one row: the two rows of a footprint share their level-1 ancestors' row, so that line is fetched by one workgroup,
// not by one per row, while a wave's neighbour in the row keeps the level-0 stream of a workgroup in runs of 2 x 64 EPL floats.
// EPL > 1 only where w is a multiple of it: a lane's pixels lie in one row, and every row starts on a multiple of EPL.
template <int EPL, bool NBR, bool UQ>
__global__ __launch_bounds__(64 * CS_WX * CS_TH) void k_cscale(CsArgs a) {
    typedef float fv __attribute__((ext_vector_type(EPL)));
    constexpr int S = SMX_CSCALE_MAX_SCALES;
    const size_t n = (size_t)a.w * a.h;
    const int tiles_x = (a.w - 1) / (64 * CS_WX * EPL) + 1;
    const int x0 = ((int)(blockIdx.x % (unsigned)tiles_x) * 64 * CS_WX + (int)(threadIdx.x % (64u * CS_WX))) * EPL;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * CS_TH + (int)(threadIdx.x / (64u * CS_WX));
    if (x0 >= a.w || y >= a.h) return;
    const size_t e0 = (size_t)y * a.w + x0;
    const int v = (int)blockIdx.y;
    const float* q = a.a[v][0] + e0;            // (not restrict: out may be this very volume)
    float* const out = a.out[v] ? a.out[v] + e0 : nullptr;
    int64_t* const keys = a.keys[v];
    float* const nbr = a.nbr[v];
    float* const uq = a.uq[v];
    const int dmin = a.dmin[v];
    const float wt0 = a.wt[0];
    int off[S][EPL];            // a pixel's ancestor inside a plane of level s (s >= 1)
    float t[S][EPL];            // the ancestor's value times the level's weight, for the label in hand
    WtaPixel<NBR, UQ> px[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        const int x = x0 + j;
#pragma unroll
        for (int s = 1; s < S; ++s) {
            off[s][j] = (y >> s) * a.ws[s] + (x >> s);
            t[s][j] = 0.0f;
        }
        px[j].load(keys, nbr, uq, n, e0 + j, true, true);
    }
    // the products of level s for label l.  Neighbouring pixels of a lane mostly share the ancestor: one load serves them
    auto level = [&](int s, int l, float (&dst)[EPL]) {
        const float* pl = a.a[v][s] + (size_t)((l >> s) - (dmin >> s)) * ((size_t)a.ws[s] * a.hs[s]);
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            if (j > 0 && off[s][j] == off[s][j - 1]) dst[j] = dst[j - 1];
            else dst[j] = a.wt[s] * pl[off[s][j]];
        }
    };
    // ... of the levels above 0 for slice z, loaded where the label's ancestor is a new one
    auto coarse = [&](int z) {
        const int l = dmin + z;
#pragma unroll
        for (int s = 1; s < S; ++s)
            if (s < a.scales && (z == 0 || (l & ((1 << s) - 1)) == 0)) level(s, l, t[s]);
    };
    auto combine = [&](fv q0) {
        fv o;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            float c = wt0 * q0[j];
#pragma unroll
            for (int s = 1; s < S; ++s)
                if (s < a.scales) c = c + t[s][j];
            o[j] = c;
        }
        return o;
    };
    auto plane = [&](int z) { return __builtin_nontemporal_load((const fv*)&q[(size_t)z * n]); };
    auto put = [&](int z, fv o) {
        if (out) __builtin_nontemporal_store(o, (fv*)&out[(size_t)z * n]);
    };
    auto single = [&](int z) {
        coarse(z);
        const fv o = combine(plane(z));
#pragma unroll
        for (int j = 0; j < EPL; ++j) px[j].step(o[j], (uint32_t)z);
        put(z, o);
    };
    {   // (the neighbour merge wants the pass's first value by itself)
        coarse(0);
        const fv o = combine(plane(0));
#pragma unroll
        for (int j = 0; j < EPL; ++j) px[j].begin(o[j], 0u);
        put(0, o);
    }
    int z = 1;
    for (; z < a.size_d && ((dmin + z) & 3) != 0; ++z) single(z);
    // Groups of four slices whose first label is a multiple of 4: level 1 changes its ancestor at the first and the third
    // slice, level 2 at the first, the levels above at the first of every 2nd, 4th group.  Their loads go out together with
    // the four level-0 loads, so no slice waits for a gather of its own.
    for (; z + 4 <= a.size_d; z += 4) {
        const int l = dmin + z;
        fv r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = plane(z + k);
        float t1[EPL];
        if (1 < a.scales) {
            level(1, l, t[1]);
            level(1, l + 2, t1);
        }
#pragma unroll
        for (int s = 2; s < S; ++s)
            if (s < a.scales && (l & ((1 << s) - 1)) == 0) level(s, l, t[s]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k == 2 && 1 < a.scales) {
#pragma unroll
                for (int j = 0; j < EPL; ++j) t[1][j] = t1[j];
            }
            const fv o = combine(r[k]);
#pragma unroll
            for (int j = 0; j < EPL; ++j) px[j].step(o[j], (uint32_t)(z + k));
            put(z + k, o);
        }
    }
    for (; z < a.size_d; ++z) single(z);
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        px[j].merge(0u);
        px[j].store(keys, nbr, uq, n, e0 + j);
    }
}

template <int EPL>
void cscale_launch_state(const CsArgs& a, int nviews, bool nbr, bool uq, hipStream_t st) {
    const size_t tiles = (size_t)((a.w - 1) / (64 * CS_WX * EPL) + 1) * (size_t)((a.h - 1) / CS_TH + 1);
    const dim3 grid((unsigned)tiles, (unsigned)nviews), block(64 * CS_WX * CS_TH);
    if (nbr && uq) hipLaunchKernelGGL((k_cscale<EPL, true, true>), grid, block, 0, st, a);
    else if (uq) hipLaunchKernelGGL((k_cscale<EPL, false, true>), grid, block, 0, st, a);
    else if (nbr) hipLaunchKernelGGL((k_cscale<EPL, true, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_cscale<EPL, false, false>), grid, block, 0, st, a);
}

}  // namespace

void pyr_down_tile(int* tw, int* th) { *tw = PYR_TW; *th = PYR_TH; }

int launch_pyr_down(const uint8_t* src, uint8_t* dst, int w, int h, int ch, hipStream_t st) {
    const int wo = (w + 1) / 2, ho = (h + 1) / 2;
    const dim3 grid((unsigned)((size_t)((wo - 1) / PYR_TW + 1) * (size_t)((ho - 1) / PYR_TH + 1))), block(PYR_TW * PYR_TH);
    if (ch == 1) hipLaunchKernelGGL(k_pyr_down<1>, grid, block, 0, st, src, dst, w, h);
    else if (ch == 3) hipLaunchKernelGGL(k_pyr_down<3>, grid, block, 0, st, src, dst, w, h);
    else hipLaunchKernelGGL(k_pyr_down<4>, grid, block, 0, st, src, dst, w, h);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_cscale_wta_pair(const smx_cscale_params* p, const float* const* agg_l, const float* const* agg_r, int w, int h, int dminl,
                           int dminr, int size_d, int64_t* keys, float* out, float* nbr, float* uq, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    // (view_slots wants one pointer a view to tell which are given: level 0's)
    const ViewSlots vs = view_slots(agg_l ? agg_l[0] : nullptr, agg_r ? agg_r[0] : nullptr, keys, out, nbr, uq, size_d, n);
    const float* const* aggs[2] = {agg_l, agg_r};
    const int dmins[2] = {dminl, dminr};
    CsArgs a = {};
    cscale_weights(p, a.wt);
    a.w = w; a.h = h; a.size_d = size_d; a.scales = p->scales;
    for (int s = 0; s < p->scales; ++s) {
        int d0, ds;
        cscale_level(w, h, 0, 1, s, &a.ws[s], &a.hs[s], &d0, &ds);
    }
    bool al16 = w % 4 == 0, al8 = w % 2 == 0;
    for (int k = 0; k < 2; ++k) {
        const int kk = k < vs.V ? k : 0;
        for (int s = 0; s < p->scales; ++s) a.a[k][s] = aggs[vs.view[kk]][s];
        a.out[k] = vs.agg[kk]; a.keys[k] = vs.keys[kk]; a.nbr[k] = vs.nbr[kk]; a.uq[k] = vs.uq[kk];
        a.dmin[k] = dmins[vs.view[kk]];
        const uintptr_t bits = (uintptr_t)a.a[k][0] | (uintptr_t)a.out[k];
        al16 = al16 && (bits & 15) == 0;
        al8 = al8 && (bits & 7) == 0;
    }
    if (al16) cscale_launch_state<4>(a, vs.V, nbr != nullptr, uq != nullptr, st);
    else if (al8) cscale_launch_state<2>(a, vs.V, nbr != nullptr, uq != nullptr, st);
    else cscale_launch_state<1>(a, vs.V, nbr != nullptr, uq != nullptr, st);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
