// smx_adjust.hip -- depth-discontinuity adjustment of a label map from the aggregated costs (the step of Mei et al. 2011 between
// the interpolation and the sub-pixel fit; not a stage of the reference: opt-in, behind the fill).  The definition is the comment
// above smx_adjust_workspace_bytes in include/smx.h and tests/adjust_ref.py, bit for bit: integers and f32 comparisons, and the
// one f32 formula of the sub-pixel map (subpixel_delta, smx_common.h).
//
//   k_adjust_round  one Jacobi round, M_k -> M_{k+1}, a thread per pixel.  A workgroup of four waves takes 64 x 4 pixels, a wave
//                   64 consecutive pixels of one row, so the map's loads and the store are whole 256-byte lines and the rows
//                   above and below are lines that the neighbouring waves load as their own.  The four neighbours are plain
//                   loads; only a pixel with a candidate touches the volume: its own cost and one cost per candidate (five
//                   gathers at most), and the two neighbours of the new slice where it changed and a sub-pixel map is given.
//                   No LDS, no barrier, no atomics.  Volume indices are 64-bit (size_d * n passes 2^32 at 4K x D512).
// A pixel changed in round k and again later has its d_sub entry written again, so what stays is the fit at its final slice; a
// changed pixel never returns to a label it had (its own cost falls strictly with every change), so "changed in some round" is
// "final label differs from the input label".
//
// Workspace (from the next 256-byte boundary on): two maps of n f32.  Round k writes d_out where it is the last, else map
// (k + a) & 1, where a = 1 if d_out == d_disp: then map 0 holds the snapshot of the input, copied there in front of the rounds.
#include "smx_api.h"
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int ADJ_TW = 64;              // columns of a workgroup = lanes of a wave
constexpr int ADJ_TH = 4;               // rows of a workgroup = its waves
constexpr int ADJ_MAX_TAU = 512;        // (ADJ_MAX_D: smx_ctx_plan.h, beside shape_ok)
constexpr int ADJ_MAX_ITER = 8;

// the slice of a labelled value, or -1.  |v| < 2^40 converts exactly; beyond it v - dmin cannot lie in 0 .. 511
__device__ inline int adj_slice(float v, int dmin, int size_d) {
    if (!(fabsf(v) < 1099511627776.0f) || v != truncf(v)) return -1;
    const long long z = (long long)v - dmin;
    return z >= 0 && z < size_d ? (int)z : -1;
}

// grid: workgroup footprints in row-major order, ADJ_TW * ADJ_TH threads.  in != out.
__global__ __launch_bounds__(ADJ_TW * ADJ_TH) void k_adjust_round(const float* __restrict__ in, float* __restrict__ out,
                                                                  const float* __restrict__ vol, float* __restrict__ sub, int mode,
                                                                  int w, int h, int dmin, int size_d, int tau_e, int vertical) {
    const int tiles_x = (w - 1) / ADJ_TW + 1;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * ADJ_TW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * ADJ_TH + (int)(threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const int64_t n = (int64_t)w * h, p = (int64_t)y * w + x;
    const float v = in[p];
    const int z = adj_slice(v, dmin, size_d);
    float take = v;
    if (z >= 0) {
        const float* col = vol + p;     // the costs of this pixel: col[slice * n]
        bool have = false;              // best holds the own cost
        float best = 0.0f;
        int zb = z;
        auto candidate = [&](bool inside, int64_t q) {
            if (!inside) return;
            const float c = in[q];
            const int zq = adj_slice(c, dmin, size_d);
            if (zq < 0 || abs(zq - z) < tau_e) return;
            if (!have) { best = col[(int64_t)z * n]; have = true; }
            const float cost = col[(int64_t)zq * n];
            if (cost < best) { best = cost; take = c; zb = zq; }
        };
        candidate(x > 0, p - 1);
        candidate(x + 1 < w, p + 1);
        if (vertical) {
            candidate(y > 0, p - w);
            candidate(y + 1 < h, p + w);
        }
        if (zb != z && sub) {
            const float nan = __builtin_nanf("");
            const float lo = zb > 0 ? col[(int64_t)(zb - 1) * n] : nan;
            const float hi = zb + 1 < size_d ? col[(int64_t)(zb + 1) * n] : nan;
            sub[p] = take + subpixel_delta(mode, best, lo, hi);
        }
    }
    out[p] = take;
}

}  // namespace

bool adjust_params_ok(const smx_adjust_params* p) {
    return p && p->tau_e >= 1 && p->tau_e <= ADJ_MAX_TAU && (p->vertical == 0 || p->vertical == 1) && p->iterations >= 1 &&
           p->iterations <= ADJ_MAX_ITER;
}

size_t adjust_workspace_bytes(int w, int h) { return 255 + 2 * sizeof(float) * (size_t)w * h; }

void adjust_tile(int* tw, int* th) { *tw = ADJ_TW; *th = ADJ_TH; }

int launch_discontinuity_adjust(const smx_adjust_params* p, const float* disp, const float* vol, float* out, int w, int h, int dmin,
                                int size_d, int mode, float* sub, void* ws, hipStream_t st) {
    const size_t n = (size_t)w * h;
    float* buf[2];
    buf[0] = reinterpret_cast<float*>(align_up((size_t)ws, 256));
    buf[1] = buf[0] + n;
    const unsigned tiles = (unsigned)((size_t)((w - 1) / ADJ_TW + 1) * (size_t)((h - 1) / ADJ_TH + 1));
    const float* cur = disp;
    int a = 0;
    if (out == disp) {
        SMX_HIP(hipMemcpyAsync(buf[0], disp, n * sizeof(float), hipMemcpyDeviceToDevice, st));
        cur = buf[0];
        a = 1;
    }
    for (int k = 0; k < p->iterations; ++k) {
        float* dst = k + 1 == p->iterations ? out : buf[(k + a) & 1];
        hipLaunchKernelGGL(k_adjust_round, dim3(tiles), dim3(ADJ_TW * ADJ_TH), 0, st, cur, dst, vol, sub, mode, w, h, dmin, size_d,
                           p->tau_e, p->vertical);
        cur = dst;
    }
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
