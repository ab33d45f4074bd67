// Mutual-information matching cost (Hirschmueller's HMI, PAMI 2008).  Not a stage of the reference: an opt-in cost that assumes
// only SOME fixed relation between the gray values of corresponding pixels and learns it from the pair, as a 256 x 256 table
// built from the joint histogram of the pixels a disparity map pairs up.  Contract (what counts, the table's order of
// operations, border cost, slice placement): include/smx.h; tests/mi_ref.py is the same in numpy.
//
// k_mi_histogram: one pixel per lane, agent-scope atomic adds into the u32 table in global memory (256 KB of counters do not
// fit the LDS), one per distinct cell of a wave with the count of the lanes that share it.  Integer sums: the same bits
// whatever the order.
//
// mi_table: the host part, in double, compiled without contraction like the rest of this library; the kernel holds no
// transcendental.
//
// k_mi_cost_pair: a pure store stream (2 * slices * w * h floats) behind a byte gather from LDS.  A workgroup loads the 64 KB
// table once and amortises it over 256 columns x MI_ROWS rows x every slice of the call x both views; the right view reads the
// same copy with the roles swapped.  The rows of the LDS copy are MI_STRIDE = 260 bytes apart: with 256 the bank of
// T[own][other] is (other / 4) % 32 whatever `own` is, and the lanes of a smooth image -- neighbouring pixels, near-equal
// values, different rows -- would all meet on one bank; with 260 it is (own + other / 4) % 32, and (other + own / 4) % 32 for
// the right view.  Per row and view the partner pixels of MI_Z slices are staged once (i16, -1 outside the image); a lane
// keeps its own pixel in a register and does, per slice, one 2-byte LDS read, one byte gather, a convert and one coalesced
// 4-byte store.  Plain stores, as in the census kernel.
#include <math.h>

#include <vector>

#include "smx_launch.h"

namespace smx {
namespace {

constexpr int MI_L = SMX_MI_LEVELS;
constexpr int MI_THREADS = 256;
constexpr int MI_COLS = 256;                                // columns (= lanes) of a cost workgroup
constexpr int MI_ROWS = 4;                                  // rows of a cost workgroup
constexpr int MI_Z = 256;                                   // slices whose partner pixels are staged at a time
constexpr int MI_STRIDE = MI_L + 4;                         // bytes between two rows of the table in LDS

__global__ __launch_bounds__(MI_THREADS) void k_mi_histogram(const uint8_t* __restrict__ il, const uint8_t* __restrict__ ir,
                                                             const float* __restrict__ map, float mark,
                                                             uint32_t* __restrict__ hist, int w, int n) {
    const int i = (int)(blockIdx.x * MI_THREADS + threadIdx.x);
    if (i >= n) return;
    const float d = map[i];
    if (d == mark) return;
    const int y = i / w, x = i - y * w;
    const int64_t xx = (int64_t)x + (int64_t)(int)d;
    if (xx < 0 || xx >= w) return;
    const uint32_t cell = (uint32_t)il[i] * MI_L + ir[(int64_t)y * w + xx];
    // one atomic per DISTINCT cell of the wave: the lanes that share the first active lane's cell leave together, and the
    // first of them adds their count (a flat region sends a whole wave to one counter; DESIGN.md 4.3s has both forms' times)
    for (;;) {
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell);
        const unsigned long long same = __ballot(cell == first);
        if (cell == first) {
            if ((int)__lane_id() == __ffsll((long long)same) - 1) atomicAdd(&hist[first], (uint32_t)__popcll(same));
            break;
        }
    }
}

__global__ __launch_bounds__(MI_THREADS) void k_mi_random_map(float* __restrict__ map, int n, int dmin, uint32_t size_d,
                                                              uint32_t seed) {
    const int i = (int)(blockIdx.x * MI_THREADS + threadIdx.x);
    if (i < n) map[i] = (float)(dmin + (int)(pm_hash(seed, 0u, (uint32_t)i, 0u) % size_d));
}

struct MiCostArgs {
    const uint8_t* table;    // [256][256], 16-byte aligned
    const uint8_t* img[2];   // left, right
    float* cost[2];          // left, right; either may be NULL
    int dmin[2];
    int w, h, s_begin, s_end, xblocks;
};

// grid (xblocks * ceil(h / MI_ROWS))
__global__ __launch_bounds__(MI_COLS) void k_mi_cost_pair(const MiCostArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tab[];      // MI_L * MI_STRIDE: more than the 64 KB a static array gets
    __shared__ int16_t other[MI_COLS + MI_Z - 1];
    const int tid = (int)threadIdx.x;
    // the table: 16 bytes of one row per lane and step, as four dwords (a row of the copy starts on a multiple of 4 only)
    const uint4* src = reinterpret_cast<const uint4*>(a.table);
    for (int i = tid; i < MI_L * MI_L / 16; i += MI_COLS) {
        const uint4 v = src[i];
        uint32_t* dst = reinterpret_cast<uint32_t*>(tab + (i >> 4) * MI_STRIDE + (i & 15) * 16);
        dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    const int x0 = (int)(blockIdx.x % (unsigned)a.xblocks) * MI_COLS;
    const int y0 = (int)(blockIdx.x / (unsigned)a.xblocks) * MI_ROWS;
    const int x = x0 + tid;
    const int64_t n = (int64_t)a.w * a.h;
    // (every bound of the loops around the barriers is uniform over the workgroup)
    for (int y = y0; y < min(y0 + MI_ROWS, a.h); ++y) {
        const int64_t row = (int64_t)y * a.w;
        for (int v = 0; v < 2; ++v) {
            if (!a.cost[v]) continue;
            const uint8_t* oth_row = a.img[1 - v] + row;
            const int own = x < a.w ? a.img[v][row + x] : 0;
            // left view: T[own][other]; right view: T[other][own]
            const uint8_t* base = v == 0 ? tab + own * MI_STRIDE : tab + own;
            const int step = v == 0 ? 1 : MI_STRIDE;
            for (int z0 = a.s_begin; z0 < a.s_end; z0 += MI_Z) {
                const int nz = min(MI_Z, a.s_end - z0);
                __syncthreads();        // the readers of the last span are through (the first time: the table is in place)
                // other[j] = the other view's pixel at x0 + d(z0) + j, d(z) = dmin + z
                const int64_t p0 = (int64_t)x0 + a.dmin[v] + z0;
                for (int j = tid; j < MI_COLS + nz - 1; j += MI_COLS) {
                    const int64_t p = p0 + j;
                    other[j] = (p >= 0 && p < a.w) ? (int16_t)oth_row[p] : (int16_t)-1;
                }
                __syncthreads();
                if (x >= a.w) continue;
                float* out = a.cost[v] + (int64_t)(z0 - a.s_begin) * n + row + x;
#pragma unroll 4
                for (int z = 0; z < nz; ++z) {
                    const int o = other[tid + z];
                    const float c = (float)base[max(o, 0) * step];
                    out[(int64_t)z * n] = o < 0 ? 255.0f : c;
                }
            }
        }
    }
}

// conv of include/smx.h over a strided vector of 256 doubles
void mi_conv(const double* in, size_t stride, double* out) {
    static const double g[7] = {1.0 / 64, 6.0 / 64, 15.0 / 64, 20.0 / 64, 15.0 / 64, 6.0 / 64, 1.0 / 64};
    for (int j = 0; j < MI_L; ++j) {
        double s = 0.0;
        for (int t = 0; t < 7; ++t) {
            const int q = j + t - 3;
            if (q >= 0 && q < MI_L) s = s + g[t] * in[(size_t)q * stride];
        }
        out[j] = s;
    }
}

void mi_conv2(std::vector<double>& m, std::vector<double>& tmp) {
    for (int i = 0; i < MI_L; ++i) mi_conv(&m[(size_t)i * MI_L], 1, &tmp[(size_t)i * MI_L]);
    double col[MI_L];
    for (int k = 0; k < MI_L; ++k) {
        mi_conv(&tmp[k], MI_L, col);
        for (int i = 0; i < MI_L; ++i) m[(size_t)i * MI_L + k] = col[i];
    }
}

void mi_entropy(double* v) {
    double t[MI_L];
    mi_conv(v, 1, t);
    for (int j = 0; j < MI_L; ++j) t[j] = -log(t[j] > 1e-12 ? t[j] : 1e-12);
    mi_conv(t, 1, v);
}

}  // namespace

void mi_table(const uint32_t* hist, uint8_t* table) {
    const size_t cells = (size_t)MI_L * MI_L;
    uint64_t n = 0;
    for (size_t i = 0; i < cells; ++i) n += hist[i];
    for (size_t i = 0; i < cells; ++i) table[i] = 0;
    if (n == 0) return;
    std::vector<double> m(cells), tmp(cells);
    double p1[MI_L], p2[MI_L];
    for (int i = 0; i < MI_L; ++i) p1[i] = p2[i] = 0.0;
    for (int i = 0; i < MI_L; ++i)
        for (int k = 0; k < MI_L; ++k) {
            const double p = (double)hist[(size_t)i * MI_L + k] / (double)n;
            m[(size_t)i * MI_L + k] = p;
            p1[i] = p1[i] + p;
            p2[k] = p2[k] + p;
        }
    mi_conv2(m, tmp);
    for (size_t i = 0; i < cells; ++i) m[i] = -log(m[i] > 1e-12 ? m[i] : 1e-12);
    mi_conv2(m, tmp);
    mi_entropy(p1);
    mi_entropy(p2);
    double lo = INFINITY, hi = 0.0;
    for (int i = 0; i < MI_L; ++i)
        for (int k = 0; k < MI_L; ++k) {
            double& c = m[(size_t)i * MI_L + k];
            c = (c - p1[i]) - p2[k];
            lo = c < lo ? c : lo;
        }
    for (size_t i = 0; i < cells; ++i) {
        m[i] = m[i] - lo;
        hi = m[i] > hi ? m[i] : hi;
    }
    if (hi == 0.0) return;
    for (size_t i = 0; i < cells; ++i) table[i] = (uint8_t)rint((m[i] * 255.0) / hi);
}

int launch_mi_histogram(const uint8_t* img_l, const uint8_t* img_r, const float* map, float mark, uint32_t* hist, int w, int h,
                        hipStream_t st) {
    const int n = w * h;
    SMX_HIP(hipMemsetAsync(hist, 0, (size_t)MI_L * MI_L * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_mi_histogram, dim3((unsigned)((n + MI_THREADS - 1) / MI_THREADS)), dim3(MI_THREADS), 0, st, img_l, img_r,
                       map, mark, hist, w, n);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_mi_random_map(float* map, int w, int h, int dmin, int size_d, uint32_t seed, hipStream_t st) {
    const int n = w * h;
    hipLaunchKernelGGL(k_mi_random_map, dim3((unsigned)((n + MI_THREADS - 1) / MI_THREADS)), dim3(MI_THREADS), 0, st, map, n, dmin,
                       (uint32_t)size_d, seed);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_mi_cost_pair(const uint8_t* table, const uint8_t* img_l, const uint8_t* img_r, float* cost_l, float* cost_r, int w,
                        int h, int dminl, int dminr, int s_begin, int s_end, hipStream_t st) {
    if (s_end <= s_begin) return SMX_OK;
    MiCostArgs a;
    a.table = table;
    a.img[0] = img_l; a.img[1] = img_r;
    a.cost[0] = cost_l; a.cost[1] = cost_r;
    a.dmin[0] = dminl; a.dmin[1] = dminr;
    a.w = w; a.h = h; a.s_begin = s_begin; a.s_end = s_end;
    a.xblocks = (w + MI_COLS - 1) / MI_COLS;
    const long long groups = (long long)a.xblocks * ((h + MI_ROWS - 1) / MI_ROWS);
    if (groups > 0x7FFFFFFFll) return fail(SMX_E_ARG, "smx_dev_mi_cost_pair: %d x %d is too many workgroups", w, h);
    static LdsLimitOnce lim;
    SMX_HIP(lim.ensure((const void*)k_mi_cost_pair, MI_L * MI_STRIDE));
    hipLaunchKernelGGL(k_mi_cost_pair, dim3((unsigned)groups), dim3(MI_COLS), MI_L * MI_STRIDE, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
