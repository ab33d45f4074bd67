// smx_patchmatch.hip -- PatchMatch stereo (Bleyer, Rhemann, Rother, BMVC 2011): a disparity plane per pixel, scored over an
// adaptive-weight window that lies in that plane, searched by random initialisation, propagation and refinement.  Not a stage
// of the reference: opt-in.  The definition is the comment above smx_pm_params in include/smx.h and tests/patchmatch_ref.py,
// bit for bit: f32, every operation rounded on its own (-ffp-contract=off), the window summed row-major in one accumulator.
//
//   k_pm_prep        the weight table (a kernel argument, computed on the host in double) into the workspace, and both views'
//                    (gray, x gradient) as one float2 a pixel: a tap's two neighbours in the other view are two 8-byte loads.
//   k_pm_init        a random plane per pixel and its cost; with plane_cost_only the cost of GIVEN planes
//                    (smx_dev_pm_plane_cost): the same walk, no search.
//   k_pm_pass        one colour of the red-black order, both views: the eight spatial candidates in ONE walk over the window
//                    (eight accumulators; the weight tab[|I_p - I_q|] and the tap's own values are shared), then the refinement
//                    steps, one walk each.  A thread per pixel of the colour; the lanes of a wave own 64 neighbouring pixels of
//                    that colour in one row, so a tap's loads of the own view are one or two lines and the other view's lie in
//                    a band of 2*64 + size_d pixels of one row.  The candidates have the other colour: nothing a thread
//                    reads is written in the launch.
//   k_pm_view        view propagation, both views, from the snapshot of the other view's planes (one device-to-device copy
//                    in front of it).
//   k_pm_finish      disp and label.
//   k_pm_sub_filled  a pair's fractional filled map (smx_dev_pm_sub_filled).
// No atomics, no wave or workgroup waits on another, one barrier a kernel (behind the table's copy into LDS).
//
// Workspace (from the next 256-byte boundary on): tab[256] f32 | ig[2][n] float2 | snapshot[2][3][n] f32.
#include "smx_api.h"
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int PM_TW = 64;              // pixels of a wave (of one colour in k_pm_pass), along x
constexpr int PM_TH = 4;               // rows of a workgroup = its waves
constexpr int PM_MAX_RADIUS = 17;
constexpr int PM_MAX_ITER = 16;
constexpr int PM_DRAWS_PER_ITER = 32;  // refinement steps a draw index leaves room for (size_d <= 2^20 takes 23)

struct PmTab { float v[256]; };

struct PmArgs {
    const float2* ig[2];        // view v: (gray, gradient) [h][w]
    float* planes[2];           // view v: a, b, d0 [3][h][w]
    float* cost[2];             // view v: m [h][w]
    const float* tab;           // [256]
    int w, h, radius, size_d;
    float dmin[2], dmax[2];
    float ms;                   // max_slope
    uint32_t seed;
    CostConst cc;
};

// (pm_hash, the counter-based hash of the draws: smx_common.h, which the random start of the MI cost shares)
__device__ inline float pm_uniform(uint32_t seed, uint32_t view, uint32_t pix, uint32_t draw) {
    return (float)(pm_hash(seed, view, pix, draw) >> 8) * 5.9604644775390625e-08f;      // 2^-24
}
// by comparisons, so that the sign of a zero is defined: a v equal to a bound stays v
__device__ inline float pm_clamp(float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; }

// rho of the tap (own values iq, gq at column qx) under disparity d; `o` is the tap's row of the other view.  A d or a
// partner outside the range (a NaN included) costs the border constant and reads column 0.
__device__ __forceinline__ float pm_rho(const float2* __restrict__ o, float iq, float gq, int qx, float d, float dmin, float dmax,
                                        int w, const CostConst& cc) {
    const float xs = (float)qx + d;
    const bool in = d >= dmin && d <= dmax && xs >= 0.0f && xs <= (float)(w - 1);
    const float xsafe = in ? xs : 0.0f;
    const float fl = floorf(xsafe);
    const int i = (int)fl;
    const int i1 = min(i + 1, w - 1);
    const float t = xsafe - fl;
    const float2 p0 = o[i], p1 = o[i1];
    const float ii = p0.x + t * (p1.x - p0.x);
    const float gi = p0.y + t * (p1.y - p0.y);
    const float t1 = fabsf(iq - ii), t2 = fabsf(gq - gi);
    const float m1 = t1 < cc.th_color ? t1 : cc.th_color;
    const float m2 = t2 < cc.th_grad ? t2 : cc.th_grad;
    const float a = cc.oma * m1;
    const float b = cc.alpha * m2;
    return in ? a + b : cc.border;
}

// The plane costs of NC planes (a[k], b[k], d0[k]) at pixel (x, y) of view v: m[k] = sum over the window, row-major, one
// accumulator a plane.  tab: the weight table in LDS.
template <int NC>
__device__ __forceinline__ void pm_costs(const PmArgs& A, const float* tab, int v, int x, int y, const float* a, const float* b,
                                         const float* d0, float* m) {
    const int w = A.w, h = A.h, r = A.radius;
    const float2* own = A.ig[v];
    const float2* oth = A.ig[v ^ 1];
    const float dmin = A.dmin[v], dmax = A.dmax[v];
    const float ip = own[(int64_t)y * w + x].x;
#pragma unroll
    for (int k = 0; k < NC; ++k) m[k] = 0.0f;
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;                  // (the same in every lane of a wave: its pixels share a row)
        const float2* orow = own + (int64_t)qy * w;
        const float2* prow = oth + (int64_t)qy * w;
        float bdy[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) bdy[k] = b[k] * (float)dy;
        for (int dx = -r; dx <= r; ++dx) {
            const int qx = x + dx;
            const bool ok = qx >= 0 && qx < w;
            const int qxc = min(max(qx, 0), w - 1);
            const float2 q = orow[qxc];
            const float wgt = tab[(int)fabsf(ip - q.x)];
            const float fdx = (float)dx;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const float d = (d0[k] + a[k] * fdx) + bdy[k];
                const float term = wgt * pm_rho(prow, q.x, q.y, qx, d, dmin, dmax, w, A.cc);
                m[k] = ok ? m[k] + term : m[k];
            }
        }
    }
}

__device__ __forceinline__ void pm_load_tab(const float* __restrict__ g, float* lds) {
    for (int k = threadIdx.x; k < 256; k += blockDim.x) lds[k] = g[k];
    __syncthreads();
}

__device__ __forceinline__ float xgrad_row(const uint8_t* __restrict__ row, int x, int w) {
    if (w < 2) return 0.0f;
    int c1, c2;
    if (x - 1 >= 0 && x + 1 < w) { c1 = row[x + 1]; c2 = row[x - 1]; }
    else if (x + 1 >= w)         { c1 = row[x];     c2 = row[x - 1]; }
    else                         { c1 = row[x + 1]; c2 = row[x];     }
    return 1.0f * (float)(c2 - c1) / 2;
}

// grid (tiles, 2 views)
__global__ __launch_bounds__(PM_TW* PM_TH) void k_pm_prep(const uint8_t* __restrict__ left, const uint8_t* __restrict__ right,
                                                           float2* __restrict__ ig, float* __restrict__ tab_out, PmTab tab, int w,
                                                           int h) {
    if (blockIdx.x == 0 && blockIdx.y == 0) tab_out[threadIdx.x] = tab.v[threadIdx.x];      // 256 threads
    const int tiles_x = (w - 1) / PM_TW + 1;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * PM_TW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * PM_TH + (int)(threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const uint8_t* row = (blockIdx.y ? right : left) + (int64_t)y * w;
    ig[(int64_t)blockIdx.y * w * h + (int64_t)y * w + x] = make_float2((float)row[x], xgrad_row(row, x, w));
}

// grid (tiles, 2 views); plane_cost_only: the planes are given, only m is written
__global__ __launch_bounds__(PM_TW* PM_TH) void k_pm_init(PmArgs A, int plane_cost_only) {
    __shared__ float tab[256];
    pm_load_tab(A.tab, tab);
    const int w = A.w, h = A.h, v = blockIdx.y;
    const int tiles_x = (w - 1) / PM_TW + 1;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * PM_TW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * PM_TH + (int)(threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, p = (int64_t)y * w + x;
    float* pl = A.planes[v];
    float a, b, d0, m;
    if (plane_cost_only) {
        a = pl[p];
        b = pl[n + p];
        d0 = pl[2 * n + p];
    } else {
        const float u0 = pm_uniform(A.seed, v, (uint32_t)p, 0), u1 = pm_uniform(A.seed, v, (uint32_t)p, 1),
                    u2 = pm_uniform(A.seed, v, (uint32_t)p, 2);
        d0 = A.dmin[v] + u0 * (float)(A.size_d - 1);
        a = (2.0f * u1 - 1.0f) * A.ms;
        b = (2.0f * u2 - 1.0f) * A.ms;
        pl[p] = a;
        pl[n + p] = b;
        pl[2 * n + p] = d0;
    }
    pm_costs<1>(A, tab, v, x, y, &a, &b, &d0, &m);
    A.cost[v][p] = m;
}

// grid (tiles of 64 x 4 pixels of the colour, 2 views)
__global__ __launch_bounds__(PM_TW* PM_TH) void k_pm_pass(PmArgs A, int it, int colour) {
    __shared__ float tab[256];
    pm_load_tab(A.tab, tab);
    const int w = A.w, h = A.h, v = blockIdx.y;
    const int tiles_x = ((w + 1) / 2 - 1) / PM_TW + 1;
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * PM_TH + (int)(threadIdx.x >> 6);
    const int j = (int)(blockIdx.x % (unsigned)tiles_x) * PM_TW + (int)(threadIdx.x & 63u);
    const int x = 2 * j + ((y + colour) & 1);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, p = (int64_t)y * w + x;
    float* pl = A.planes[v];
    const float dmin = A.dmin[v], dmax = A.dmax[v];
    float a = pl[p], b = pl[n + p], d0 = pl[2 * n + p], m = A.cost[v][p];

    // spatial propagation: (-1,0) (1,0) (0,-1) (0,1) (-5,0) (5,0) (0,-5) (0,5), all of the other colour
    float ca[8], cb[8], cd[8], cm[8];
    bool cok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = k & 4 ? 5 : 1, sg = k & 1 ? s : -s;
        const int ddx = k & 2 ? 0 : sg, ddy = k & 2 ? sg : 0;
        const int nx = x + ddx, ny = y + ddy;
        const bool inside = nx >= 0 && nx < w && ny >= 0 && ny < h;
        const int64_t q = inside ? (int64_t)ny * w + nx : p;
        ca[k] = pl[q];
        cb[k] = pl[n + q];
        cd[k] = (pl[2 * n + q] + ca[k] * (float)(-ddx)) + cb[k] * (float)(-ddy);
        cok[k] = inside && cd[k] >= dmin && cd[k] <= dmax;
    }
    pm_costs<8>(A, tab, v, x, y, ca, cb, cd, cm);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool take = cok[k] && cm[k] < m;
        a = take ? ca[k] : a;
        b = take ? cb[k] : b;
        d0 = take ? cd[k] : d0;
        m = take ? cm[k] : m;
    }

    // refinement: the perturbation halves every step; each step starts from what the step before left
    float dd = (float)(A.size_d - 1) * 0.5f, ds = A.ms * 0.5f;
    for (int k = 0; dd >= 0.1f; ++k) {
        const uint32_t base = 3u + 3u * (uint32_t)(it * PM_DRAWS_PER_ITER + k);
        const float r0 = 2.0f * pm_uniform(A.seed, v, (uint32_t)p, base) - 1.0f;
        const float r1 = 2.0f * pm_uniform(A.seed, v, (uint32_t)p, base + 1u) - 1.0f;
        const float r2 = 2.0f * pm_uniform(A.seed, v, (uint32_t)p, base + 2u) - 1.0f;
        const float dn = pm_clamp(d0 + r0 * dd, dmin, dmax);
        const float an = pm_clamp(a + r1 * ds, -A.ms, A.ms);
        const float bn = pm_clamp(b + r2 * ds, -A.ms, A.ms);
        float c;
        pm_costs<1>(A, tab, v, x, y, &an, &bn, &dn, &c);
        const bool take = c < m;
        a = take ? an : a;
        b = take ? bn : b;
        d0 = take ? dn : d0;
        m = take ? c : m;
        dd = dd * 0.5f;
        ds = ds * 0.5f;
    }
    pl[p] = a;
    pl[n + p] = b;
    pl[2 * n + p] = d0;
    A.cost[v][p] = m;
}

// grid (tiles, 2 views); snap: [2][3][n], the planes of both views before this launch
__global__ __launch_bounds__(PM_TW* PM_TH) void k_pm_view(PmArgs A, const float* __restrict__ snap) {
    __shared__ float tab[256];
    pm_load_tab(A.tab, tab);
    const int w = A.w, h = A.h, v = blockIdx.y;
    const int tiles_x = (w - 1) / PM_TW + 1;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * PM_TW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * PM_TH + (int)(threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, p = (int64_t)y * w + x;
    float* pl = A.planes[v];
    const float d0 = pl[2 * n + p];
    const int xo = min(max((int)floorf(((float)x + d0) + 0.5f), 0), w - 1);
    const float* so = snap + (int64_t)(v ^ 1) * 3 * n + (int64_t)y * w + xo;
    const float an = -so[0], bn = -so[n], dn = -so[2 * n];
    if (!(dn >= A.dmin[v] && dn <= A.dmax[v])) return;
    float c;
    pm_costs<1>(A, tab, v, x, y, &an, &bn, &dn, &c);
    if (c < A.cost[v][p]) {
        pl[p] = an;
        pl[n + p] = bn;
        pl[2 * n + p] = dn;
        A.cost[v][p] = c;
    }
}

// grid (tiles, 2 views)
__global__ __launch_bounds__(PM_TW* PM_TH) void k_pm_finish(PmArgs A, float* __restrict__ disp, float* __restrict__ label) {
    const int w = A.w, h = A.h, v = blockIdx.y;
    const int tiles_x = (w - 1) / PM_TW + 1;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * PM_TW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * PM_TH + (int)(threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, p = (int64_t)y * w + x;
    const float d0 = A.planes[v][2 * n + p];
    disp[v * n + p] = d0;
    label[v * n + p] = pm_clamp(floorf(d0 + 0.5f), A.dmin[v], A.dmax[v]);
}

// the rule of k_subpixel_pair (smx_subpix.hip): fill_occlusion's test, (int)kept < dminl, defined for every float
__global__ __launch_bounds__(256) void k_pm_sub_filled(const float* __restrict__ disp, const float* __restrict__ kept,
                                                       const float* __restrict__ filled, size_t n, int dminl,
                                                       float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float o = kept[i];
    const bool dropped = fabsf(o) <= 3.402823466e38f && trunc((double)o) < (double)dminl;
    out[i] = dropped ? filled[i] : disp[i];
}

struct PmWs {
    float* tab;
    float2* ig;
    float* snap;
};
PmWs pm_carve(void* ws, size_t n) {
    PmWs s;
    s.tab = reinterpret_cast<float*>(align_up((size_t)ws, 256));
    s.ig = reinterpret_cast<float2*>(s.tab + 256);
    s.snap = reinterpret_cast<float*>(s.ig + 2 * n);
    return s;
}

PmArgs pm_args(const smx_params* p, const smx_pm_params* pm, const PmWs& s, float* planes, float* cost, int w, int h, int size_d,
               int dminl, int dminr) {
    const size_t n = (size_t)w * h;
    PmArgs A;
    A.ig[0] = s.ig;
    A.ig[1] = s.ig + n;
    A.planes[0] = planes;
    A.planes[1] = planes + 3 * n;
    A.cost[0] = cost;
    A.cost[1] = cost + n;
    A.tab = s.tab;
    A.w = w;
    A.h = h;
    A.radius = pm->radius;
    A.size_d = size_d;
    A.dmin[0] = (float)dminl;
    A.dmin[1] = (float)dminr;
    A.dmax[0] = (float)(dminl + size_d - 1);
    A.dmax[1] = (float)(dminr + size_d - 1);
    A.ms = (float)pm->max_slope;
    A.seed = pm->seed;
    A.cc = make_cost_const(p);
    return A;
}

void pm_prep(const smx_pm_params* pm, const PmWs& s, const uint8_t* left, const uint8_t* right, int w, int h, dim3 grid,
             hipStream_t st) {
    PmTab tab;
    pm_weights(pm, tab.v);
    hipLaunchKernelGGL(k_pm_prep, grid, dim3(PM_TW * PM_TH), 0, st, left, right, s.ig, s.tab, tab, w, h);
}

}  // namespace

bool pm_params_ok(const smx_pm_params* p) {
    return p && p->radius >= 0 && p->radius <= PM_MAX_RADIUS && p->gamma > 0.0 && p->gamma <= 1.7976931348623157e308 &&
           p->iterations >= 1 && p->iterations <= PM_MAX_ITER && p->max_slope >= 0.0 && p->max_slope <= 8.0;
}

void pm_weights(const smx_pm_params* p, float* tab) {
    for (int k = 0; k < 256; ++k) tab[k] = (float)exp(-(double)k / p->gamma);
}

uint32_t pm_hash_host(uint32_t seed, uint32_t view, uint32_t pix, uint32_t draw) { return pm_hash(seed, view, pix, draw); }

size_t pm_workspace_bytes(int w, int h) { return 255 + 256 * sizeof(float) + (size_t)w * h * (2 * sizeof(float2) + 6 * sizeof(float)); }

void pm_tile(int* tw, int* th) { *tw = PM_TW; *th = PM_TH; }

int launch_pm_sub_filled(const float* disp, const float* kept, const float* filled, size_t n, int dminl, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_pm_sub_filled, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, disp, kept, filled, n, dminl, out);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_patchmatch_pair(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                           int size_d, int dminl, int dminr, float* planes, float* cost, float* disp, float* label, void* ws,
                           hipStream_t st) {
    const size_t n = (size_t)w * h;
    const PmWs s = pm_carve(ws, n);
    const PmArgs A = pm_args(p, pm, s, planes, cost, w, h, size_d, dminl, dminr);
    const unsigned rows = (unsigned)((h - 1) / PM_TH + 1);
    const dim3 all((unsigned)((w - 1) / PM_TW + 1) * rows, 2), half((unsigned)(((w + 1) / 2 - 1) / PM_TW + 1) * rows, 2),
        block(PM_TW * PM_TH);
    pm_prep(pm, s, left, right, w, h, all, st);
    hipLaunchKernelGGL(k_pm_init, all, block, 0, st, A, 0);
    for (int it = 0; it < pm->iterations; ++it) {
        hipLaunchKernelGGL(k_pm_pass, half, block, 0, st, A, it, it & 1);
        hipLaunchKernelGGL(k_pm_pass, half, block, 0, st, A, it, (it & 1) ^ 1);
        SMX_HIP(hipMemcpyAsync(s.snap, planes, 6 * n * sizeof(float), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_pm_view, all, block, 0, st, A, (const float*)s.snap);
    }
    hipLaunchKernelGGL(k_pm_finish, all, block, 0, st, A, disp, label);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                         int size_d, int dminl, int dminr, const float* planes, float* cost, void* ws, hipStream_t st) {
    const size_t n = (size_t)w * h;
    const PmWs s = pm_carve(ws, n);
    const PmArgs A = pm_args(p, pm, s, const_cast<float*>(planes), cost, w, h, size_d, dminl, dminr);
    const dim3 all((unsigned)((w - 1) / PM_TW + 1) * (unsigned)((h - 1) / PM_TH + 1), 2), block(PM_TW * PM_TH);
    pm_prep(pm, s, left, right, w, h, all, st);
    hipLaunchKernelGGL(k_pm_init, all, block, 0, st, A, 1);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
