// smx_perm.hip -- the information permeability filter (Cigla & Alatan 2013; not a stage of the reference: opt-in).  The
// definition is the comment above smx_perm_params in include/smx.h and tests/perm_ref.py, bit for bit: every product and sum of
// the four recurrences rounded to f32 on its own, in the order of the definition, whatever the launch geometry.
//
//   k_perm_weights  the permeabilities of up to two guides from the table t[256] (a kernel argument, staged in LDS): mu_v as a
//                   plane [h][w], mu_h TRANSPOSED, [w][h], because the horizontal pass reads it with a lane per row.
//   k_perm_h        the horizontal pass of a chunk of slices of up to two views.  The sequential direction is the contiguous one:
//                   a wave owns 64 rows of one slice, a lane one of them, and walks them in tiles of 32 columns that the wave
//                   loads row segment by row segment (128 B runs, two rows an instruction) and transposes through LDS padded to
//                   33 floats a row: the store of a segment and a lane's walk along its row both touch every bank of a 32-lane
//                   group once.  First sweep: LR, left to right, into the scratch slab; second sweep: RL, right to left, with C
//                   and LR read again, Hh out.
//   k_perm_v        the vertical pass: a lane owns a column of one slice, so every access is coalesced as it is.  TB downwards
//                   into the scratch slab, then BT upwards with Hh and TB read again (by the lane that wrote them), out.
//
// Either pass may write over its input: a tile (a column) is read for the last time before it is written, by the wave (the lane)
// that writes it.  No atomics, no grid-wide synchronisation, no flags between workgroups, no transcendental, no
// floating-point division.
// The winners come from wta_launch (smx_wta.h) over the filtered slices of each chunk.
//
// Must be compiled with -ffp-contract=off.
#include "smx_api.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int PW_PX = 8;        // pixels of a lane of the weight kernel
constexpr int PH_ROWS = 64;     // rows of a wave of the horizontal pass: a lane each
constexpr int PH_COLS = 32;     // columns of a tile of it: 16.5 KiB of LDS a wave
constexpr int PV_COLS = 256;    // columns of a workgroup of the vertical pass
constexpr int P_U = 8;          // rows a lane of the vertical pass loads ahead of its recurrence

struct PermTable { float t[256]; };

struct PermWeightArgs {
    const uint8_t* guide[2];
    float* muhT[2];             // [w][h]; column 0 is written as 0 and never read
    float* muv[2];              // [h][w]; row 0 likewise
    int w, h;
};

template <int CH>
__device__ inline int perm_diff(const uint8_t* a, const uint8_t* b) {
    int d = 0;
#pragma unroll
    for (int c = 0; c < (CH == 1 ? 1 : 3); ++c) {       // (alpha is ignored)
        const int e = (int)a[c] - (int)b[c];
        const int m = e < 0 ? -e : e;
        d = m > d ? m : d;
    }
    return d;
}

// grid (runs of 256 * PW_PX pixels, views)
template <int CH>
__global__ __launch_bounds__(256) void k_perm_weights(PermWeightArgs a, PermTable tab) {
    __shared__ float t[256];
    {   // (a kernel argument is not indexed by the lane: every lane picks its entry out of the uniform values)
        float mine = 0.0f;
#pragma unroll
        for (int k = 0; k < 256; ++k) mine = (int)threadIdx.x == k ? tab.t[k] : mine;
        t[threadIdx.x] = mine;
    }
    __syncthreads();
    const int v = (int)blockIdx.y;
    const uint8_t* I = a.guide[v];
    const size_t n = (size_t)a.w * a.h;
    const size_t first = (size_t)blockIdx.x * (256 * PW_PX) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < PW_PX; ++k) {
        const size_t id = first + (size_t)k * 256;
        if (id >= n) break;
        const int y = (int)(id / (unsigned)a.w), x = (int)(id - (size_t)y * a.w);
        const uint8_t* px = I + id * CH;
        float mh = 0.0f, mv = 0.0f;
        if (x >= 1) mh = t[perm_diff<CH>(px, px - CH)];
        if (y >= 1) mv = t[perm_diff<CH>(px, px - (size_t)a.w * CH)];
        a.muhT[v][(size_t)x * a.h + y] = mh;
        a.muv[v][id] = mv;
    }
}

struct PermArgs {
    const float* in[2];         // per view: the first slice of the chunk
    float* out[2];              // may be in[]
    float* scr[2];              // the chunk's scratch slab
    const float* mu[2];         // muhT (horizontal pass) or muv (vertical pass)
    int w, h;
};

// grid (tiles of PH_ROWS rows, slices of the chunk, views); one wave a workgroup.  Per tile and sweep every global load -- the
// tile's row segments, two a wave instruction, and the lane's PH_COLS weights -- goes out before the first wait, and the walk is
// straight-line code: a column past the image leaves the recurrence as it is and is never stored.
__global__ __launch_bounds__(PH_ROWS) void k_perm_h(PermArgs a) {
    __shared__ float tc[PH_ROWS][PH_COLS + 1], tl[PH_ROWS][PH_COLS + 1];
    const int lane = (int)threadIdx.x, v = (int)blockIdx.z;
    const int w = a.w, h = a.h;
    const int y0 = (int)blockIdx.x * PH_ROWS;
    const int rows = h - y0 < PH_ROWS ? h - y0 : PH_ROWS;
    const size_t base = ((size_t)blockIdx.y * h + y0) * w;
    const float* in = a.in[v] + base;       // (not restrict: out may be in)
    float* out = a.out[v] + base;
    float* scr = a.scr[v] + base;
    // this lane's row of the transposed weights; a lane past the image walks the last row and stores nothing
    const float* mu = a.mu[v] + (y0 + lane < h ? y0 + lane : h - 1);
    const int last = (w - 1) / PH_COLS * PH_COLS;
    const int sr = lane / PH_COLS, sc = lane % PH_COLS;     // this lane's row of the pair and column in a segment instruction
    constexpr int SEG = PH_ROWS * PH_COLS / 64;             // segment instructions of a tile
    // (no branch around a load: a row or a column past the image reads the last one inside it, into a cell that is not used,
    // so that all of a tile's loads are in flight together)
    auto load = [&](const float* src, float (*tile)[PH_COLS + 1], int x0) {
        const int xc = x0 + sc < w ? x0 + sc : w - 1;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int r = i * (64 / PH_COLS) + sr;
            tile[r][sc] = src[(size_t)(r < rows ? r : rows - 1) * w + xc];
        }
    };
    auto store = [&](float* dst, int x0) {
        const bool on = x0 + sc < w;
        float t[SEG];
#pragma unroll
        for (int i = 0; i < SEG; ++i) t[i] = tc[i * (64 / PH_COLS) + sr][sc];
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int r = i * (64 / PH_COLS) + sr;
            if (on && r < rows) dst[(size_t)r * w + x0 + sc] = t[i];
        }
    };
    // the weights of the steps INTO columns x0 + off .. of this lane's row (clamped: what lies past the image is not used)
    auto weights = [&](int x0, int off, float (&m)[PH_COLS]) {
#pragma unroll
        for (int j = 0; j < PH_COLS; ++j) {
            const int x = x0 + j + off;
            m[j] = mu[(size_t)(x < w ? x : w - 1) * h];
        }
    };
    float lr = 0.0f;
    for (int x0 = 0; x0 <= last; x0 += PH_COLS) {
        float m[PH_COLS];
        weights(x0, 0, m);
        load(in, tc, x0);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PH_COLS; ++j) {
            const int x = x0 + j;
            const float c = tc[lane][j];
            const float p = m[j] * lr;
            const float s = c + p;
            lr = x >= w ? lr : x == 0 ? c : s;
            tc[lane][j] = lr;
        }
        __syncthreads();
        store(scr, x0);
        __syncthreads();
    }
    float rl = 0.0f;
    for (int x0 = last; x0 >= 0; x0 -= PH_COLS) {
        float m[PH_COLS];
        weights(x0, 1, m);
        load(in, tc, x0);
        load(scr, tl, x0);
        __syncthreads();
#pragma unroll
        for (int j = PH_COLS - 1; j >= 0; --j) {
            const int x = x0 + j;
            const float c = tc[lane][j];
            const float p = m[j] * rl;
            const float s = c + p;
            rl = x >= w ? rl : x == w - 1 ? c : s;
            const float t = tl[lane][j] + rl;
            tc[lane][j] = t - c;
        }
        __syncthreads();
        store(out, x0);
        __syncthreads();
    }
}

// grid (runs of PV_COLS columns, slices of the chunk, views)
__global__ __launch_bounds__(PV_COLS) void k_perm_v(PermArgs a) {
    const int w = a.w, h = a.h, v = (int)blockIdx.z;
    const int x = (int)blockIdx.x * PV_COLS + (int)threadIdx.x;
    if (x >= w) return;
    const size_t base = (size_t)blockIdx.y * h * w + x;
    const float* in = a.in[v] + base;       // (not restrict: out may be in)
    float* out = a.out[v] + base;
    float* scr = a.scr[v] + base;
    const float* mu = a.mu[v] + x;
    float tb = 0.0f;
    for (int y0 = 0; y0 < h; y0 += P_U) {
        float c[P_U], m[P_U];
#pragma unroll
        for (int k = 0; k < P_U; ++k) {
            const int y = y0 + k;
            c[k] = y < h ? in[(size_t)y * w] : 0.0f;
            m[k] = y < h ? mu[(size_t)y * w] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < P_U; ++k) {
            const int y = y0 + k;
            if (y < h) {
                const float p = m[k] * tb;
                tb = y == 0 ? c[k] : c[k] + p;
                scr[(size_t)y * w] = tb;
            }
        }
    }
    float bt = 0.0f;
    for (int y0 = (h - 1) / P_U * P_U; y0 >= 0; y0 -= P_U) {
        float c[P_U], m[P_U], t[P_U];
#pragma unroll
        for (int k = 0; k < P_U; ++k) {
            const int y = y0 + k;
            c[k] = y < h ? in[(size_t)y * w] : 0.0f;
            t[k] = y < h ? scr[(size_t)y * w] : 0.0f;
            m[k] = y + 1 < h ? mu[(size_t)(y + 1) * w] : 0.0f;
        }
#pragma unroll
        for (int k = P_U - 1; k >= 0; --k) {
            const int y = y0 + k;
            if (y < h) {
                const float p = m[k] * bt;
                bt = y == h - 1 ? c[k] : c[k] + p;
                const float s = t[k] + bt;
                out[(size_t)y * w] = s - c[k];
            }
        }
    }
}

// the floats of one view's plane
inline size_t plane_bytes(int w, int h) { return (size_t)w * h * sizeof(float); }

}  // namespace

// Per view: the two weight planes, and per slice in flight a scratch plane (LR, then TB) and a plane of the filtered slice for
// the calls that keep no volume.  Sized for those: a call with d_out gets by with less.
size_t perm_workspace_bytes(int w, int h, int nslices, int nviews) {
    return (size_t)nviews * plane_bytes(w, h) * (2 + 2 * (size_t)nslices);
}

int perm_chunk(int w, int h, int nviews, size_t ws_bytes, int count, bool own_out, int max_chunk) {
    const size_t per = (size_t)nviews * plane_bytes(w, h);
    if (ws_bytes / per < 2) return 0;
    size_t k = (ws_bytes / per - 2) / (own_out ? 2 : 1);
    if (k > (size_t)count) k = (size_t)count;
    if (k > 65535) k = 65535;           // (the slices of a chunk are a grid dimension)
    if (max_chunk > 0 && k > (size_t)max_chunk) k = (size_t)max_chunk;
    return (int)k;
}

int launch_perm_wta_pair(const float* table, const float* vol_l, const float* vol_r, const uint8_t* guide_l, const uint8_t* guide_r,
                         int ch, int w, int h, int size_d, int64_t* keys, float* out, float* nbr, float* uq, void* ws, int chunk,
                         hipStream_t st) {
    const size_t n = (size_t)w * h;
    const float* vols[2] = {vol_l, vol_r};
    const uint8_t* guides[2] = {guide_l, guide_r};
    const int both = vol_l && vol_r ? 1 : 0;
    // view k of the V given ones; with both views the outputs hold the left view first, a single view lies at the front
    int V = 0;
    const float* vin[2] = {};
    float* vout[2] = {};
    int64_t* vkeys[2] = {};
    float *vnbr[2] = {}, *vuq[2] = {};
    PermWeightArgs wa = {};
    wa.w = w; wa.h = h;
    float* const wsf = (float*)ws;
    for (int view = 0; view < 2; ++view) {
        if (!vols[view]) continue;
        const size_t slot = both ? (size_t)view : 0;
        vin[V] = vols[view];
        vout[V] = out ? out + slot * size_d * n : nullptr;
        vkeys[V] = keys ? keys + slot * n : nullptr;
        vnbr[V] = nbr ? nbr + slot * 3 * n : nullptr;
        vuq[V] = uq ? uq + slot * 3 * n : nullptr;
        wa.guide[V] = guides[view];
        wa.muhT[V] = wsf + (size_t)V * 2 * n;
        wa.muv[V] = wa.muhT[V] + n;
        ++V;
    }
    float* const scr = wsf + (size_t)V * 2 * n;                  // [V][chunk][n]
    float* const own = scr + (size_t)V * chunk * n;              // [V][chunk][n], used where out is NULL
    PermTable tab;
    for (int k = 0; k < 256; ++k) tab.t[k] = table[k];
    {
        const dim3 grid((unsigned)((n - 1) / (256 * PW_PX) + 1), (unsigned)V), block(256);
        if (ch == 1) hipLaunchKernelGGL(k_perm_weights<1>, grid, block, 0, st, wa, tab);
        else if (ch == 3) hipLaunchKernelGGL(k_perm_weights<3>, grid, block, 0, st, wa, tab);
        else hipLaunchKernelGGL(k_perm_weights<4>, grid, block, 0, st, wa, tab);
        SMX_HIP(hipGetLastError());
    }
    for (int s0 = 0; s0 < size_d; s0 += chunk) {
        const int cnt = s0 + chunk < size_d ? chunk : size_d - s0;
        PermArgs ha = {}, va = {};
        ha.w = va.w = w; ha.h = va.h = h;
        const float* q[2] = {};
        for (int k = 0; k < V; ++k) {
            float* dst = vout[k] ? vout[k] + (size_t)s0 * n : own + (size_t)k * chunk * n;
            ha.in[k] = vin[k] + (size_t)s0 * n;
            ha.out[k] = va.out[k] = dst;
            va.in[k] = dst;
            ha.scr[k] = va.scr[k] = scr + (size_t)k * chunk * n;
            ha.mu[k] = wa.muhT[k];
            va.mu[k] = wa.muv[k];
            q[k] = dst;
        }
        hipLaunchKernelGGL(k_perm_h, dim3((unsigned)((h - 1) / PH_ROWS + 1), (unsigned)cnt, (unsigned)V), dim3(PH_ROWS), 0, st, ha);
        hipLaunchKernelGGL(k_perm_v, dim3((unsigned)((w - 1) / PV_COLS + 1), (unsigned)cnt, (unsigned)V), dim3(PV_COLS), 0, st, va);
        SMX_HIP(hipGetLastError());
        if (keys)
            if (int rc = wta_launch(WTA_NATURAL, V, q, vkeys, nbr ? vnbr : nullptr, uq ? vuq : nullptr, w, h, n, cnt, s0, nullptr, 0,
                                    s0 == 0, st))
                return rc;
    }
    return SMX_OK;
}

}  // namespace smx
