// smx_cgf.hip -- the colour-guided filter aggregation (smx_dev_cgf_wta_pair; not a stage of the reference): the guided
// filter of He et al. with an RGB guide, i.e. the 3 x 3 covariance of the guide per window, over materialised cost volumes,
// with the project's winner-take-all pass behind it.  A path of its own next to the multi-kernel gray path (k_rowscan,
// k_colscan, k_ab, k_q_wta of smx_kernels.hip); the definition is the comment above smx_cgf_workspace_bytes in
// include/smx.h and tests/cgf_ref.py, bit for bit.
//
// Numerical contract as in smx_kernels.hip: -ffp-contract=off, every operation rounded on its own in source order, prefix
// sums in the sequential order `acc = v + acc` from -0.0f, left to right then top to bottom.
//
// Workspace (planes of n = w*h floats from the next 256-byte boundary on; V = views of the call, c = slices in flight):
//   G  V * 9 planes   per view mu_r, mu_g, mu_b, then A, B, C, D, E, F of (Sigma + eps I)^-1 = (A B C; B D E; C E F)
//   W  V * max(9, 8c) planes
//        guidance phase:  per view the 9 integrals of I_r, I_g, I_b, rr, rg, rb, gg, gb, bb
//        slice phase:     P = V * 4c planes, slice z of view v at (v*c + z) * 4: integrals of p, I_r p, I_g p, I_b p
//                         Q = V * 4c planes behind P, same order: a_r, a_g, a_b, b, then their integrals in place
// The views are contiguous in every region, so the scans, which touch no caller buffer, see one stack of planes.
#include "smx_common.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int CGF_TX = 32;      // columns of a row-scan tile
constexpr int CGF_TY = 64;      // rows of a band: one lane per row in the scan
constexpr int CGF_NP = 4;       // planes per workgroup of the row scan, one wave each

struct CgfViews {
    const uint8_t* rgb[2];
    const float* cost[2];       // slice s of the call at cost[(s - s_begin) * n]
    int64_t* keys[2];
    float* agg[2];
    float* nbr[2];
    float* uq[2];
};

static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// ---- box mean from an integral image: box_taps / box_eval of smx_kernels.hip ------------------------------------------------
struct Taps {
    int64_t i11, i10, i01, i00;
    bool hx, hy;
    float area;
};

__device__ __forceinline__ Taps taps_of(int x, int y, int w, int h, int R) {
    // (y + R, x + R overflow only for R near INT_MAX: clamp the radius, a window beyond the image is the image)
    R = min(R, max(w, h));
    const int ymin = max(-1, y - R - 1), ymax = min(h - 1, y + R);
    const int xmin = max(-1, x - R - 1), xmax = min(w - 1, x + R);
    Taps t;
    t.hx = xmin >= 0;
    t.hy = ymin >= 0;
    t.i11 = (int64_t)ymax * w + xmax;
    t.i10 = (int64_t)ymax * w + (t.hx ? xmin : 0);
    t.i01 = (int64_t)(t.hy ? ymin : 0) * w + xmax;
    t.i00 = (int64_t)(t.hy ? ymin : 0) * w + (t.hx ? xmin : 0);
    t.area = (float)((xmax - xmin) * (ymax - ymin));
    return t;
}

__device__ __forceinline__ float box(const float* __restrict__ S, const Taps& t) {
    float val = S[t.i11];
    if (t.hx) val -= S[t.i10];
    if (t.hy) val -= S[t.i01];
    if (t.hx && t.hy) val += S[t.i00];
    return val / t.area;
}

// ---- guidance: the nine planes to integrate ------------------------------------------------------------------------------------
// grid (ceil(n / 256), V)
__global__ void k_cgf_prep(CgfViews v, int ch, float* __restrict__ W, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint8_t* px = v.rgb[blockIdx.y] + (int64_t)ch * k;
    const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
    float* o = W + (int64_t)blockIdx.y * 9 * n + k;
    o[0] = r;
    o[n] = g;
    o[2 * n] = b;
    o[3 * n] = r * r;       // (products of two bytes: exact)
    o[4 * n] = r * g;
    o[5 * n] = r * b;
    o[6 * n] = g * g;
    o[7 * n] = g * b;
    o[8 * n] = b * b;
}

// ---- row scan ---------------------------------------------------------------------------------------------------------------------
// A workgroup of CGF_NP waves takes a band of 64 rows of CGF_NP planes.  Per tile of 32 columns all four waves load (128-byte
// row segments, every load of the tile in flight before the first LDS store), wave k then scans plane k with lane r on row r
// -- the sequential chain, its carry in a register across the tiles -- and all four store.  The tiles are padded to 33
// floats, so the lanes of a scan hit 32 different banks.
//   COST = false: planes [4g, 4g + 4) of a stack of `nplanes`, in place
//   COST = true:  group g is slice z = g % c of view g / c: p is loaded once, the guide's three bytes beside it, and the four
//                 planes p, I_r p, I_g p, I_b p go to planes [4g, 4g + 4) of `out`
// grid (bands * groups)
template <bool COST>
__global__ __launch_bounds__(64 * CGF_NP) void k_cgf_rowscan(CgfViews v, int ch, int c, float* out, int w, int h, int nplanes) {
    __shared__ float t[CGF_NP][CGF_TY][CGF_TX + 1];
    const int bands = (h + CGF_TY - 1) / CGF_TY;
    const int g = blockIdx.x / bands;
    const int y0 = (blockIdx.x - g * bands) * CGF_TY;
    const int rows = min(CGF_TY, h - y0);
    const int64_t n = (int64_t)w * h;
    const int tid = threadIdx.x, lc = tid & 31, lr = tid >> 5;        // 8 rows of 32 columns per pass
    const int wave = tid >> 6, lane = tid & 63;
    const int np = COST ? CGF_NP : min(CGF_NP, nplanes - g * CGF_NP);
    float* o = out + (int64_t)g * CGF_NP * n + (int64_t)y0 * w;
    const float* p = nullptr;
    const uint8_t* rgb = nullptr;
    if (COST) {
        const int view = g / c, z = g - view * c;
        p = v.cost[view] + (int64_t)z * n + (int64_t)y0 * w;
        rgb = v.rgb[view] + (int64_t)y0 * w * ch;
    }
    float acc = -0.0f;
    for (int x0 = 0; x0 < w; x0 += CGF_TX) {
        const int cols = min(CGF_TX, w - x0);
        if (COST) {
            float pv[8], cr[8], cg[8], cb[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = 8 * i + lr;
                const bool on = r < rows && lc < cols;
                const int64_t e = on ? (int64_t)r * w + x0 + lc : 0;
                pv[i] = p[e];
                cr[i] = (float)rgb[e * ch];
                cg[i] = (float)rgb[e * ch + 1];
                cb[i] = (float)rgb[e * ch + 2];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = 8 * i + lr;
                t[0][r][lc] = pv[i];
                t[1][r][lc] = cr[i] * pv[i];
                t[2][r][lc] = cg[i] * pv[i];
                t[3][r][lc] = cb[i] * pv[i];
            }
        } else {
            for (int k = 0; k < np; ++k) {
                float pv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int r = 8 * i + lr;
                    const bool on = r < rows && lc < cols;
                    pv[i] = o[(int64_t)k * n + (on ? (int64_t)r * w + x0 + lc : 0)];
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) t[k][8 * i + lr][lc] = pv[i];
            }
        }
        __syncthreads();
        if (wave < np && lane < rows) {
            for (int j = 0; j < cols; ++j) {
                acc = t[wave][lane][j] + acc;
                t[wave][lane][j] = acc;
            }
        }
        __syncthreads();
        for (int k = 0; k < np; ++k) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int r = 8 * i + lr;
                if (r < rows && lc < cols) o[(int64_t)k * n + (int64_t)r * w + x0 + lc] = t[k][r][lc];
            }
        }
        __syncthreads();
    }
}

// ---- column scan, in place: one lane per (plane, column) of a stack; 8 loads in flight around the chain ------------------------
__global__ void k_cgf_colscan(float* buf, int w, int h, int64_t nplanes) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= nplanes * w) return;
    const int64_t plane = gid / w;
    float* p = buf + plane * ((int64_t)w * h) + (gid - plane * w);
    float acc = -0.0f;
    int y = 0;
    for (; y + 8 <= h; y += 8) {
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = p[(int64_t)(y + k) * w];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            acc = s[k] + acc;
            p[(int64_t)(y + k) * w] = acc;
        }
    }
    for (; y < h; ++y) {
        acc = p[(int64_t)y * w] + acc;
        p[(int64_t)y * w] = acc;
    }
}

// ---- guidance: means, covariance, the inverse in double -----------------------------------------------------------------------
// grid (ceil(w / 256), h, V)
__global__ void k_cgf_guid(const float* __restrict__ W, float* __restrict__ G, int w, int h, int R, double eps) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int64_t n = (int64_t)w * h, id = (int64_t)y * w + x;
    const float* S = W + (int64_t)blockIdx.z * 9 * n;
    float* o = G + (int64_t)blockIdx.z * 9 * n + id;
    const Taps t = taps_of(x, y, w, h, R);
    const float mr = box(S, t), mg = box(S + n, t), mb = box(S + 2 * n, t);
    const float mrr = box(S + 3 * n, t), mrg = box(S + 4 * n, t), mrb = box(S + 5 * n, t);
    const float mgg = box(S + 6 * n, t), mgb = box(S + 7 * n, t), mbb = box(S + 8 * n, t);
    const float prr = mr * mr, prg = mr * mg, prb = mr * mb, pgg = mg * mg, pgb = mg * mb, pbb = mb * mb;
    const float vrr = mrr - prr, vrg = mrg - prg, vrb = mrb - prb, vgg = mgg - pgg, vgb = mgb - pgb, vbb = mbb - pbb;
    const double a = (double)vrr + eps, b = (double)vrg, c = (double)vrb;
    const double d = (double)vgg + eps, e = (double)vgb, f = (double)vbb + eps;
    const double A = d * f - e * e, B = c * e - b * f, C = b * e - c * d;
    const double D = a * f - c * c, E = b * c - a * e, F = a * d - b * b;
    const double det = (a * A + b * B) + c * C;
    o[0] = mr;
    o[n] = mg;
    o[2 * n] = mb;
    o[3 * n] = (float)(A / det);
    o[4 * n] = (float)(B / det);
    o[5 * n] = (float)(C / det);
    o[6 * n] = (float)(D / det);
    o[7 * n] = (float)(E / det);
    o[8 * n] = (float)(F / det);
}

// ---- a_r, a_g, a_b, b of a slice ------------------------------------------------------------------------------------------------
// grid (ceil(w / 256), h, V * c); plane group blockIdx.z = view * c + z
__global__ void k_cgf_ab(const float* __restrict__ P, const float* __restrict__ G, float* __restrict__ Q, int c, int w, int h, int R) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int64_t n = (int64_t)w * h, id = (int64_t)y * w + x;
    const int view = blockIdx.z / c;
    const float* S = P + (int64_t)blockIdx.z * 4 * n;
    const float* g = G + (int64_t)view * 9 * n + id;
    float* o = Q + (int64_t)blockIdx.z * 4 * n + id;
    const Taps t = taps_of(x, y, w, h, R);
    const float mp = box(S, t), mrp = box(S + n, t), mgp = box(S + 2 * n, t), mbp = box(S + 3 * n, t);
    const float mr = g[0], mg = g[n], mb = g[2 * n];
    const float A = g[3 * n], B = g[4 * n], C = g[5 * n], D = g[6 * n], E = g[7 * n], F = g[8 * n];
    const float pr = mr * mp, pg = mg * mp, pb = mb * mp;
    const float cr = mrp - pr, cg = mgp - pg, cb = mbp - pb;
    const float ar0 = A * cr, ar1 = B * cg, ar2 = C * cb;
    const float ag0 = B * cr, ag1 = D * cg, ag2 = E * cb;
    const float ab0 = C * cr, ab1 = E * cg, ab2 = F * cb;
    const float ar = (ar0 + ar1) + ar2, ag = (ag0 + ag1) + ag2, ab = (ab0 + ab1) + ab2;
    const float s0 = ar * mr, s1 = ag * mg, s2 = ab * mb;
    const float bk = mp - ((s0 + s1) + s2);
    o[0] = ar;
    o[n] = ag;
    o[2 * n] = ab;
    o[3 * n] = bk;
}

// ---- q and the running winner-take-all over the chunk's slices -----------------------------------------------------------------
// grid (ceil(w / 256), h, V).  One lane per pixel, WtaPixel as in k_q_wta.
template <bool NBR, bool UQ>
__global__ void k_cgf_q_wta(CgfViews v, int ch, const float* __restrict__ Q, int c, int w, int h, int count, int slice0,
                            int agg0, int R) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const int view = blockIdx.z;
    const int64_t n = (int64_t)w * h, id = (int64_t)y * w + x;
    const uint8_t* px = v.rgb[view] + id * ch;
    const float Ir = (float)px[0], Ig = (float)px[1], Ib = (float)px[2];
    const float* S = Q + (int64_t)view * c * 4 * n;
    float* agg = v.agg[view];
    const Taps t = taps_of(x, y, w, h, R);
    WtaPixel<NBR, UQ> wp;
    wp.load(v.keys[view], v.nbr[view], v.uq[view], (size_t)n, (size_t)id, true, false);
    for (int z = 0; z < count; ++z) {
        const float* Sz = S + (int64_t)z * 4 * n;
        const float ar = box(Sz, t), ag = box(Sz + n, t), ab = box(Sz + 2 * n, t), bb = box(Sz + 3 * n, t);
        const float q0 = ar * Ir, q1 = ag * Ig, q2 = ab * Ib;
        const float q = ((q0 + q1) + q2) + bb;
        if (z == 0) wp.begin(q, (uint32_t)slice0);
        else wp.step(q, (uint32_t)(slice0 + z));
        if (agg) agg[(int64_t)(agg0 + z) * n + id] = q;
    }
    wp.merge((uint32_t)slice0);
    wp.store(v.keys[view], v.nbr[view], v.uq[view], (size_t)n, (size_t)id);
}

constexpr int CGF_MAX_CHUNK = 16384;    // (grid.z of k_cgf_ab is V * c)

size_t plane_bytes(int w, int h) { return (size_t)w * h * sizeof(float); }

}  // namespace

size_t cgf_workspace_bytes(int w, int h, int nslices, int nviews) {
    const size_t c = (size_t)(nslices < CGF_MAX_CHUNK ? nslices : CGF_MAX_CHUNK);
    return 255 + (size_t)nviews * (9 + (8 * c > 9 ? 8 * c : 9)) * plane_bytes(w, h);
}

// slices in flight that a workspace of ws_bytes holds (0: not even one), whatever its alignment
int cgf_chunk(int w, int h, int nviews, size_t ws_bytes, int count, int max_chunk) {
    if (ws_bytes < cgf_workspace_bytes(w, h, 1, nviews)) return 0;
    const size_t planes = (ws_bytes - 255) / plane_bytes(w, h) / (size_t)nviews;       // per view, >= 18
    size_t c = (planes - 9) / 8;
    if (c > (size_t)count) c = (size_t)count;
    if (max_chunk > 0 && c > (size_t)max_chunk) c = (size_t)max_chunk;
    if (c > (size_t)CGF_MAX_CHUNK) c = CGF_MAX_CHUNK;
    return (int)c;
}

int launch_cgf_wta_pair(const smx_params* p, const uint8_t* rgb_l, const uint8_t* rgb_r, int ch, const float* cost_l,
                        const float* cost_r, int w, int h, int s_begin, int s_end, int64_t* keys, float* agg, float* nbr,
                        float* uq, void* ws, int chunk, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    const int count = s_end - s_begin, R = p->radius;
    CgfViews v = {};
    const ViewSlots s = view_slots(cost_l, cost_r, keys, agg, nbr, uq, count, n);
    const int V = s.V;
    const uint8_t* rgbs[2] = {rgb_l, rgb_r};
    const float* costs[2] = {cost_l, cost_r};
    s.put(v);
    for (int k = 0; k < V; ++k) { v.rgb[k] = rgbs[s.view[k]]; v.cost[k] = costs[s.view[k]]; }
    float* G = reinterpret_cast<float*>(align_up((size_t)ws, 256));
    float* W = G + (int64_t)V * 9 * n;
    const dim3 b256(256), bscan(64 * CGF_NP);
    const int bands = (h + CGF_TY - 1) / CGF_TY;
    auto scan_in_place = [&](float* stack, int64_t nplanes) -> int {
        const int64_t groups = (nplanes + CGF_NP - 1) / CGF_NP;
        hipLaunchKernelGGL(k_cgf_rowscan<false>, dim3((unsigned)(bands * groups)), bscan, 0, st, v, ch, 1, stack, w, h, (int)nplanes);
        SMX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cgf_colscan, dim3(cdiv(nplanes * w, 256)), b256, 0, st, stack, w, h, nplanes);
        SMX_HIP(hipGetLastError());
        return SMX_OK;
    };
    // guidance, once per call
    hipLaunchKernelGGL(k_cgf_prep, dim3(cdiv(n, 256), (unsigned)V), b256, 0, st, v, ch, W, n);
    SMX_HIP(hipGetLastError());
    if (int rc = scan_in_place(W, (int64_t)V * 9)) return rc;
    hipLaunchKernelGGL(k_cgf_guid, dim3(cdiv(w, 256), (unsigned)h, (unsigned)V), b256, 0, st, W, G, w, h, R, p->eps);
    SMX_HIP(hipGetLastError());
    // the slices, `chunk` at a time
    for (int z0 = 0; z0 < count; z0 += chunk) {
        const int c = count - z0 < chunk ? count - z0 : chunk;
        float* P = W;
        float* Q = W + (int64_t)V * c * 4 * n;
        CgfViews vc = v;
        for (int k = 0; k < V; ++k) vc.cost[k] = v.cost[k] + (int64_t)z0 * n;
        hipLaunchKernelGGL(k_cgf_rowscan<true>, dim3((unsigned)((int64_t)bands * V * c)), bscan, 0, st, vc, ch, c, P, w, h, V * c * 4);
        SMX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cgf_colscan, dim3(cdiv((int64_t)V * c * 4 * w, 256)), b256, 0, st, P, w, h, (int64_t)V * c * 4);
        SMX_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_cgf_ab, dim3(cdiv(w, 256), (unsigned)h, (unsigned)(V * c)), b256, 0, st, P, G, Q, c, w, h, R);
        SMX_HIP(hipGetLastError());
        if (int rc = scan_in_place(Q, (int64_t)V * c * 4)) return rc;
        const dim3 grid(cdiv(w, 256), (unsigned)h, (unsigned)V);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, b256, 0, st, vc, ch, Q, c, w, h, c, s_begin + z0, z0, R);
        };
        if (nbr && uq) go(k_cgf_q_wta<true, true>);
        else if (uq) go(k_cgf_q_wta<false, true>);
        else if (nbr) go(k_cgf_q_wta<true, false>);
        else go(k_cgf_q_wta<false, false>);
        SMX_HIP(hipGetLastError());
    }
    return SMX_OK;
}

}  // namespace smx
