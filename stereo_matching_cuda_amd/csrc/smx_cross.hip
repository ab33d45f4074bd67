// smx_cross.hip -- cross-based aggregation (Zhang, Lu, Lafruit 2009, as Mei et al. 2011 use it behind AD-Census; not a stage
// of the reference): per pixel a colour-adaptive support region made of four arms, built once per view from the guide, and
// per slice `iterations` two-pass sums over it, alternating horizontal-first and vertical-first, with the project's
// winner-take-all pass behind them.  The definition is the comment above smx_cross_workspace_bytes in include/smx.h and
// tests/cross_ref.py, bit for bit: everything is an exact integer in u32, so any summation order gives the same bits.
//
// Decomposition: a row kernel and a column kernel with a u32 plane between them (not one fused walker per iteration).
//   k_cross_arms  the four arms of every pixel of both views, one u32 per pixel
//   k_cross_h     sums over the horizontal arm: a workgroup takes 128 columns of one row with 64 columns of halo either
//                 side, one element per lane, an inclusive scan over the workgroup (DPP inside a wave, one LDS word per
//                 wave to join them), H = P[x + r] - P[x - l - 1] from LDS
//   k_cross_v     sums over the vertical arm: one lane per column walks down the rows with a running column prefix (u32,
//                 may wrap: differences stay exact) in an LDS ring of 2 * l1 + 2 rows, and emits row y - l1 as
//                 Q[y0 + d] - Q[y0 - u - 1].  A lane touches only its own column of the ring: no barrier.
// Either kernel reads f32 cost (through the clamp), u16, u32 or the constant 1, and writes the raw sum (u32 or u16) or the
// rounded quotient by the area (u16, or f32 q for the last iteration).  The two area planes of a view are the same two
// passes over the constant 1.
//
// Workspace (from the next 256-byte boundary on; n = w*h, V = views of the call, c = slices in flight):
//   ARMS  V planes of n u32
//   AREA  V * 2 planes of n u16: per view area_HV, area_VH
//   A, B  V * c planes of n u16 each: the values between iterations, ping-pong
//   T     V * c planes of n u32: the sums of an iteration's first pass (and of the area passes)
//   Q     V * c planes of n f32: q of the chunk, unless the caller's d_agg takes it
#include "smx_api.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int CROSS_MAX_L1 = 63;
constexpr int ARM_TX = 256;             // columns of a workgroup of the arms kernel
constexpr int H_STRIP = 128;            // columns a workgroup of k_cross_h emits
constexpr int H_HALO = 64;              // > CROSS_MAX_L1: columns staged either side of the strip
constexpr int V_TX = 64;                // columns of a workgroup of k_cross_v: one wave
constexpr int V_ROWS = 4;               // rows whose loads are in flight around the prefix chain
constexpr int CROSS_MAX_CHUNK = 16384;  // (grid.y of the sum kernels is V * c)

enum { IN_COST = 0, IN_U16 = 1, IN_U32 = 2, IN_ONE = 3 };
enum { OUT_RAW32 = 0, OUT_RAW16 = 1, OUT_DIV16 = 2, OUT_DIVF = 3 };

// What a sum kernel reads and writes: per view a stack of planes, plane z of the chunk at element z * n
struct CrossIo {
    const void* in[2];
    void* out[2];
    const uint16_t* area[2];    // OUT_DIV*: the area plane of the iteration's order
    int in_kind, out_kind;
};

static inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__device__ inline uint32_t clamp_cost(float c) { return c >= 0.0f ? (c <= 255.0f ? (uint32_t)(int)c : 255u) : 0u; }

__device__ inline uint32_t load_v(const void* p, int kind, int64_t i) {
    if (kind == IN_COST) return 16u * clamp_cost(static_cast<const float*>(p)[i]);
    if (kind == IN_U16) return static_cast<const uint16_t*>(p)[i];
    if (kind == IN_U32) return static_cast<const uint32_t*>(p)[i];
    return 1u;
}

// i: the element of the output stack, ia: the pixel (the element of the view's area plane)
__device__ inline void store_v(void* p, int kind, const uint16_t* area, int64_t i, int64_t ia, uint32_t s) {
    if (kind == OUT_RAW32) { static_cast<uint32_t*>(p)[i] = s; return; }
    if (kind == OUT_RAW16) { static_cast<uint16_t*>(p)[i] = (uint16_t)s; return; }
    const uint32_t a = area[ia];
    const uint32_t v = (2u * s + a) / (2u * a);         // (a >= 1: the pixel itself; 2 s + a < 2^28)
    if (kind == OUT_DIV16) static_cast<uint16_t*>(p)[i] = (uint16_t)v;
    else static_cast<float*>(p)[i] = (float)v * 0.0625f;
}

// ---- arms -------------------------------------------------------------------------------------------------------------------
// a pixel as r | g << 8 | b << 16 (a gray guide: the byte three times, which gives the same distance)
__device__ inline uint32_t load_px(const uint8_t* g, int ch, int64_t i) {
    const uint8_t* p = g + i * ch;
    const uint32_t r = p[0];
    if (ch == 1) return r | r << 8 | r << 16;
    return r | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

__device__ inline int cdist(uint32_t a, uint32_t b) {
    const int d0 = abs((int)(a & 255u) - (int)(b & 255u));
    const int d1 = abs((int)((a >> 8) & 255u) - (int)((b >> 8) & 255u));
    const int d2 = abs((int)(a >> 16) - (int)(b >> 16));
    return max(d0, max(d1, d2));
}

// does q, j steps from p and one step from prev, extend p's arm?
__device__ inline bool arm_ok(uint32_t q, uint32_t p, uint32_t prev, int j, const smx_cross_params& cp) {
    const int dp = cdist(q, p);
    return dp < cp.tau1 && cdist(q, prev) < cp.tau1 && (j <= cp.l2 || dp < cp.tau2);
}

// grid (strips * h, V), ARM_TX threads; `strips` strips of ARM_TX columns.  The row segment with its l1 halo goes through LDS
// for the horizontal arms; the vertical arms read the guide strided.
__global__ __launch_bounds__(ARM_TX) void k_cross_arms(const uint8_t* g0, const uint8_t* g1, int ch, smx_cross_params cp,
                                                       uint32_t* __restrict__ arms, int w, int h, int strips) {
    __shared__ uint32_t row[ARM_TX + 2 * CROSS_MAX_L1];
    const int tid = threadIdx.x, l1 = cp.l1;
    const int y = (int)(blockIdx.x / (unsigned)strips);
    const int x0 = (int)(blockIdx.x - (unsigned)y * (unsigned)strips) * ARM_TX;
    const uint8_t* g = blockIdx.y ? g1 : g0;
    const int64_t n = (int64_t)w * h, base = (int64_t)y * w;
    for (int i = tid; i < ARM_TX + 2 * l1; i += ARM_TX) {
        const int x = x0 - l1 + i;
        row[i] = x >= 0 && x < w ? load_px(g, ch, base + x) : 0u;
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x >= w) return;
    const uint32_t p = row[tid + l1];
    int l = 0, r = 0, u = 0, d = 0;
    uint32_t prev = p;
    for (int j = 1; j <= l1 && x - j >= 0; ++j) {
        const uint32_t q = row[tid + l1 - j];
        if (!arm_ok(q, p, prev, j, cp)) break;
        l = j;
        prev = q;
    }
    prev = p;
    for (int j = 1; j <= l1 && x + j < w; ++j) {
        const uint32_t q = row[tid + l1 + j];
        if (!arm_ok(q, p, prev, j, cp)) break;
        r = j;
        prev = q;
    }
    prev = p;
    for (int j = 1; j <= l1 && y - j >= 0; ++j) {
        const uint32_t q = load_px(g, ch, base + x - (int64_t)j * w);
        if (!arm_ok(q, p, prev, j, cp)) break;
        u = j;
        prev = q;
    }
    prev = p;
    for (int j = 1; j <= l1 && y + j < h; ++j) {
        const uint32_t q = load_px(g, ch, base + x + (int64_t)j * w);
        if (!arm_ok(q, p, prev, j, cp)) break;
        d = j;
        prev = q;
    }
    arms[(int64_t)blockIdx.y * n + base + x] = (uint32_t)l | (uint32_t)r << 8 | (uint32_t)u << 16 | (uint32_t)d << 24;
}

// ---- sums over the horizontal arm ----------------------------------------------------------------------------------------------
// inclusive prefix sum over the 64 lanes of a wave: row_shr:1, 2, 4, 8 inside each row of 16 lanes, then row_bcast:15 into
// rows 1 and 3 and row_bcast:31 into rows 2 and 3 (a lane without a source adds the `old` value 0)
__device__ inline uint32_t wave_scan(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
    return x;
}

// grid (strips * h, V * c), 256 threads; `strips` strips of H_STRIP columns.  Lane t holds column x0 - H_HALO + t (0 outside
// the image), so x - l - 1 >= x0 - H_HALO and x + r < x0 + H_STRIP + H_HALO stay inside the workgroup's 256 prefix values.
__global__ __launch_bounds__(256) void k_cross_h(CrossIo io, const uint32_t* __restrict__ arms, int c, int w, int h, int strips) {
    __shared__ uint32_t P[2 * H_HALO + H_STRIP];
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int y = (int)(blockIdx.x / (unsigned)strips);
    const int x0 = (int)(blockIdx.x - (unsigned)y * (unsigned)strips) * H_STRIP;
    const int v = (int)blockIdx.y / c, z = (int)blockIdx.y - v * c;
    const int64_t n = (int64_t)w * h, base = (int64_t)z * n + (int64_t)y * w;
    const int x = x0 - H_HALO + tid;
    const bool in_image = x >= 0 && x < w;
    uint32_t s = in_image ? load_v(v ? io.in[1] : io.in[0], io.in_kind, base + x) : 0u;
    s = wave_scan(s);
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    for (int k = 0; k < wave; ++k) s += wsum[k];
    P[tid] = s;
    __syncthreads();
    if (tid < H_HALO || tid >= H_HALO + H_STRIP || !in_image) return;
    const uint32_t a = arms[(int64_t)v * n + (int64_t)y * w + x];
    const int l = (int)(a & 255u), r = (int)((a >> 8) & 255u);
    store_v(v ? io.out[1] : io.out[0], io.out_kind, v ? io.area[1] : io.area[0], base + x, (int64_t)y * w + x,
            P[tid + r] - P[tid - l - 1]);
}

// ---- sums over the vertical arm --------------------------------------------------------------------------------------------------
// grid (ceil(w / V_TX), V * c), V_TX threads, rr * V_TX words of dynamic LDS with rr = 2 * l1 + 2 ring rows.  Row y0 = y - l1
// is emitted once row y is in the ring: y0 + d <= y, and y0 - u - 1 >= y - rr + 1 is the oldest row still there.
__global__ __launch_bounds__(V_TX) void k_cross_v(CrossIo io, const uint32_t* __restrict__ arms, int c, int w, int h, int l1) {
    extern __shared__ uint32_t ring[];
    const int tid = threadIdx.x, x = (int)blockIdx.x * V_TX + tid;
    if (x >= w) return;             // (no barrier below: a lane reads what it wrote itself)
    const int rr = 2 * l1 + 2;
    const int v = (int)blockIdx.y / c, z = (int)blockIdx.y - v * c;
    const int64_t n = (int64_t)w * h, base = (int64_t)z * n + x;
    const uint32_t* am = arms + (int64_t)v * n + x;
    const void* in = v ? io.in[1] : io.in[0];
    void* out = v ? io.out[1] : io.out[0];
    const uint16_t* area = v ? io.area[1] : io.area[0];
    uint32_t q = 0u;
    int wr = 0;                     // y mod rr
    for (int yb = 0; yb < h + l1; yb += V_ROWS) {
        uint32_t vin[V_ROWS], a[V_ROWS];
#pragma unroll
        for (int k = 0; k < V_ROWS; ++k) {
            const int y = yb + k, y0 = y - l1;
            vin[k] = y < h ? load_v(in, io.in_kind, base + (int64_t)y * w) : 0u;
            a[k] = y0 >= 0 && y0 < h ? am[(int64_t)y0 * w] : 0u;
        }
#pragma unroll
        for (int k = 0; k < V_ROWS; ++k) {
            const int y = yb + k, y0 = y - l1;
            if (y < h) {
                q += vin[k];
                ring[wr * V_TX + tid] = q;
            }
            if (y0 >= 0 && y0 < h) {
                const int u = (int)((a[k] >> 16) & 255u), d = (int)(a[k] >> 24);
                int ih = wr - (l1 - d);
                ih = ih < 0 ? ih + rr : ih;
                uint32_t s = ring[ih * V_TX + tid];
                if (y0 - u - 1 >= 0) {
                    int il = wr - (l1 + u + 1);
                    il = il < 0 ? il + rr : il;
                    s -= ring[il * V_TX + tid];
                }
                store_v(out, io.out_kind, area, base + (int64_t)y0 * w, (int64_t)y0 * w + x, s);
            }
            wr = wr + 1 == rr ? 0 : wr + 1;
        }
    }
}

size_t cells(int w, int h) { return (size_t)w * h; }      // of one plane

int launch_h(const CrossIo& io, const uint32_t* arms, int V, int c, int w, int h, hipStream_t st) {
    const int strips = (int)cdiv(w, H_STRIP);
    hipLaunchKernelGGL(k_cross_h, dim3((unsigned)((int64_t)strips * h), (unsigned)(V * c)), dim3(256), 0, st, io, arms, c, w, h, strips);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_v(const CrossIo& io, const uint32_t* arms, int V, int c, int w, int h, int l1, hipStream_t st) {
    const size_t lds = (size_t)(2 * l1 + 2) * V_TX * sizeof(uint32_t);      // <= 32 KiB
    hipLaunchKernelGGL(k_cross_v, dim3(cdiv(w, V_TX), (unsigned)(V * c)), dim3(V_TX), lds, st, io, arms, c, w, h, l1);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

// order 0: horizontal first, order 1: vertical first
int launch_two_pass(int order, const CrossIo& first, const CrossIo& second, const uint32_t* arms, int V, int c, int w, int h,
                    int l1, hipStream_t st) {
    if (int rc = order == 0 ? launch_h(first, arms, V, c, w, h, st) : launch_v(first, arms, V, c, w, h, l1, st)) return rc;
    return order == 0 ? launch_v(second, arms, V, c, w, h, l1, st) : launch_h(second, arms, V, c, w, h, st);
}

int launch_arms(const smx_cross_params* p, const uint8_t* const* guide, int V, int ch, int w, int h, uint32_t* arms,
                hipStream_t st) {
    const int strips = (int)cdiv(w, ARM_TX);
    hipLaunchKernelGGL(k_cross_arms, dim3((unsigned)((int64_t)strips * h), (unsigned)V), dim3(ARM_TX), 0, st, guide[0],
                       guide[V - 1], ch, *p, arms, w, h, strips);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace

bool cross_params_ok(const smx_cross_params* p) {
    return p && p->l1 >= 1 && p->l1 <= CROSS_MAX_L1 && p->l2 >= 0 && p->l2 <= p->l1 && p->tau2 >= 1 && p->tau2 <= p->tau1 &&
           p->tau1 <= 256 && p->iterations >= 1 && p->iterations <= 4;
}

size_t cross_workspace_bytes(int w, int h, int nslices, int nviews) {
    const size_t c = (size_t)(nslices < CROSS_MAX_CHUNK ? nslices : CROSS_MAX_CHUNK);
    return 255 + (size_t)nviews * (8 + 12 * c) * cells(w, h);
}

// slices in flight that a workspace of ws_bytes holds (0: not even one), whatever its alignment
int cross_chunk(int w, int h, int nviews, size_t ws_bytes, int count, int max_chunk) {
    if (ws_bytes < cross_workspace_bytes(w, h, 1, nviews)) return 0;
    const size_t per_cell = (ws_bytes - 255) / cells(w, h) / (size_t)nviews;       // >= 20
    size_t c = (per_cell - 8) / 12;
    if (c > (size_t)count) c = (size_t)count;
    if (max_chunk > 0 && c > (size_t)max_chunk) c = (size_t)max_chunk;
    if (c > (size_t)CROSS_MAX_CHUNK) c = CROSS_MAX_CHUNK;
    return (int)c;
}

int launch_cross_arms(const smx_cross_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch, int w, int h,
                      uint32_t* arms, hipStream_t st) {
    const uint8_t* guide[2];
    int V = 0;
    if (guide_l) guide[V++] = guide_l;
    if (guide_r) guide[V++] = guide_r;
    return launch_arms(p, guide, V, ch, w, h, arms, st);
}

int launch_cross_wta_pair(const smx_cross_params* p, const uint8_t* guide_l, const uint8_t* guide_r, int ch, const float* cost_l,
                          const float* cost_r, int w, int h, int s_begin, int s_end, int64_t* keys, float* agg, float* nbr,
                          float* uq, void* ws, int chunk, hipStream_t st) {
    const int64_t n = (int64_t)w * h;
    const int count = s_end - s_begin, l1 = p->l1;
    const ViewSlots s = view_slots(cost_l, cost_r, keys, agg, nbr, uq, count, n);
    const int V = s.V;
    const uint8_t* guide[2] = {};
    const float* cost[2] = {};
    const uint8_t* guides[2] = {guide_l, guide_r};
    const float* costs[2] = {cost_l, cost_r};
    for (int k = 0; k < V; ++k) { guide[k] = guides[s.view[k]]; cost[k] = costs[s.view[k]]; }
    uint8_t* base = reinterpret_cast<uint8_t*>(align_up((size_t)ws, 256));
    uint32_t* ARMS = reinterpret_cast<uint32_t*>(base);
    uint16_t* AREA = reinterpret_cast<uint16_t*>(base + (size_t)V * 4 * n);
    uint16_t* A = reinterpret_cast<uint16_t*>(base + (size_t)V * 8 * n);
    uint16_t* B = A + (int64_t)V * chunk * n;
    uint32_t* T = reinterpret_cast<uint32_t*>(B + (int64_t)V * chunk * n);
    float* Q = reinterpret_cast<float*>(T + (int64_t)V * chunk * n);

    // the support regions, once per call: the arms, then the two area planes of every view
    if (int rc = launch_arms(p, guide, V, ch, w, h, ARMS, st)) return rc;
    for (int order = 0; order < 2; ++order) {
        CrossIo first = {}, second = {};
        first.in_kind = IN_ONE;
        first.out_kind = OUT_RAW32;
        second.in_kind = IN_U32;
        second.out_kind = OUT_RAW16;
        for (int k = 0; k < V; ++k) {
            first.out[k] = T + (int64_t)k * n;
            second.in[k] = T + (int64_t)k * n;
            second.out[k] = AREA + ((int64_t)k * 2 + order) * n;
        }
        if (int rc = launch_two_pass(order, first, second, ARMS, V, 1, w, h, l1, st)) return rc;
    }
    // the slices, `chunk` at a time
    for (int z0 = 0; z0 < count; z0 += chunk) {
        const int c = count - z0 < chunk ? count - z0 : chunk;
        const float* q[2] = {};
        for (int k = 0; k < V; ++k) q[k] = s.agg[k] ? s.agg[k] + (int64_t)z0 * n : Q + (int64_t)k * c * n;
        for (int i = 0; i < p->iterations; ++i) {
            const int order = i & 1;
            const bool last = i + 1 == p->iterations;
            uint16_t* from = i & 1 ? A : B;     // (iteration 0 reads the cost)
            uint16_t* to = i & 1 ? B : A;
            CrossIo first = {}, second = {};
            first.in_kind = i == 0 ? IN_COST : IN_U16;
            first.out_kind = OUT_RAW32;
            second.in_kind = IN_U32;
            second.out_kind = last ? OUT_DIVF : OUT_DIV16;
            for (int k = 0; k < V; ++k) {
                first.in[k] = i == 0 ? static_cast<const void*>(cost[k] + (int64_t)z0 * n) : from + (int64_t)k * c * n;
                first.out[k] = T + (int64_t)k * c * n;
                second.in[k] = T + (int64_t)k * c * n;
                second.out[k] = last ? static_cast<void*>(const_cast<float*>(q[k])) : to + (int64_t)k * c * n;
                second.area[k] = AREA + ((int64_t)k * 2 + order) * n;
            }
            if (int rc = launch_two_pass(order, first, second, ARMS, V, c, w, h, l1, st)) return rc;
        }
        if (int rc = wta_launch(WTA_NATURAL, V, q, s.keys, nbr ? s.nbr : nullptr, uq ? s.uq : nullptr, w, h, (size_t)n, c,
                                s_begin + z0, nullptr, 0, false, st))
            return rc;
    }
    return SMX_OK;
}

}  // namespace smx
