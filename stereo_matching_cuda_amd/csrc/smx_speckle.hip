// Speckle removal: a connected-component filter on a disparity map (OpenCV's filterSpeckles rule; not a stage of the
// reference: opt-in, between the LR check and the scan-line fill).  Contract (which pixels count, which neighbours are
// joined, what is rewritten): include/smx.h.
//
// Connected-component labelling as a union-find forest over the image: label[p] <= p is p's parent (the image-linear
// index of a pixel of the same component), a root has label[r] == r, and the root of a component ends up as the smallest
// index in it, whatever the order of the atomics -- so the result does not depend on scheduling.  Four launches on one
// stream; the kernel boundaries are the only ordering between them (no grid barrier, no workgroup waits for another):
//   k_speckle_tile   one workgroup per 64 x 16 tile, labelled in LDS: the runs of a row by ballots (no atomics), the
//                    joins between rows by a union-find with LDS atomicMin; then label[p] = the tile-local root of p and
//                    size[root] = the root's pixels inside the tile.  No global atomics.
//   k_speckle_seams  one lane per pixel on a tile's right / bottom edge: if it is joined to its neighbour across the
//                    seam, the two roots are united (lock-free: atomicMin of the larger root's entry to the smaller one,
//                    repeated on what the atomic returns).  Every access to the label plane is an agent-scope atomic.
//   k_speckle_sum    one lane per tile-local root that lost its rank: the tile's count is added to size[final root] with
//                    one integer atomicAdd (exact in any order), and label[root] is shortened to the final root.
//   k_speckle_apply  one lane per pixel: root, size, new_val or the input.
// Every loop ends on its own: a walk towards a root strictly decreases the index (label[p] <= p holds from the first
// store on, an atomicMin only lowers an entry), and a walk that met anything else would stop at once.
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int SPK_TW = 64;                      // tile columns = lanes of a wave
constexpr int SPK_TH = 16;                      // tile rows
constexpr int SPK_WAVES = 4;
constexpr int SPK_THREADS = 64 * SPK_WAVES;
constexpr int SPK_ROWS = SPK_TH / SPK_WAVES;    // rows of a wave: ty = wave + j * SPK_WAVES
constexpr uint32_t SPK_NONE = 0xFFFFFFFFu;      // label of a pixel that does not count

// fill_occlusion's validity test on a finite value: (float)(int)v >= vmin, the conversion saturating as the hardware's
__device__ inline bool speckle_counts(float v, float vmin) {
    if (!(fabsf(v) <= 3.402823466e38f)) return false;       // NaN, +-inf
    const float t = v >= 2147483648.0f ? 2147483648.0f : v < -2147483648.0f ? -2147483648.0f : (float)(int)v;
    return t >= vmin;
}

__device__ inline uint32_t lds_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// unite the trees of a and b in an LDS forest
__device__ inline void lds_unite(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {
        for (uint32_t p; (p = lds_load(lab + a)) < a;) a = p;
        for (uint32_t p; (p = lds_load(lab + b)) < b;) b = p;
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old >= a) return;       // a was still a root: it hangs under b now
        a = old;                    // somebody else hung a under old < a first: unite old and b
    }
}

__global__ __launch_bounds__(SPK_THREADS) void k_speckle_tile(const float* __restrict__ disp, uint32_t* __restrict__ label,
                                                              uint32_t* __restrict__ size, int w, int h, float vmin,
                                                              float max_diff) {
    __shared__ float sv[SPK_TW * SPK_TH];           // the tile; NaN = does not count (or lies outside the image)
    __shared__ uint32_t lab[SPK_TW * SPK_TH];       // tile-local forest: lab[i] <= i
    __shared__ uint32_t cnt[SPK_TW * SPK_TH];       // pixels of a tile-local root
    __shared__ uint64_t rrow[SPK_TH + 1];           // bit x of rrow[y]: (x, y) is joined to (x + 1, y)
    const int tiles_x = (w - 1) / SPK_TW + 1;       // w >= 1; w + SPK_TW - 1 would overflow next to 2^31
    const int x0 = (int)(blockIdx.x % tiles_x) * SPK_TW, y0 = (int)(blockIdx.x / tiles_x) * SPK_TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float nan = __int_as_float(0x7FC00000);

    float v[SPK_ROWS];
#pragma unroll
    for (int j = 0; j < SPK_ROWS; ++j) {
        const int ty = wave + j * SPK_WAVES, x = x0 + lane, y = y0 + ty;
        float d = nan;
        if (x < w && y < h) {
            d = disp[(size_t)y * w + x];
            if (!speckle_counts(d, vmin)) d = nan;
        }
        v[j] = d;
        sv[ty * SPK_TW + lane] = d;
        cnt[ty * SPK_TW + lane] = 0;
    }
    if (threadIdx.x == 0) rrow[SPK_TH] = 0;
    __syncthreads();

    // the runs of a row: a pixel starts one unless it is joined to its left neighbour; every pixel points at the start
    uint64_t rm[SPK_ROWS], dm[SPK_ROWS];
    int head[SPK_ROWS];
#pragma unroll
    for (int j = 0; j < SPK_ROWS; ++j) {
        const int ty = wave + j * SPK_WAVES, i = ty * SPK_TW + lane;
        const float right = lane < SPK_TW - 1 ? sv[i + 1] : nan;
        const float below = ty < SPK_TH - 1 ? sv[i + SPK_TW] : nan;
        rm[j] = __ballot(fabsf(v[j] - right) <= max_diff);       // false for a NaN on either side
        dm[j] = __ballot(fabsf(v[j] - below) <= max_diff);
        const bool counts = v[j] == v[j];
        const uint64_t heads = __ballot(counts && !(lane > 0 && ((rm[j] >> (lane - 1)) & 1)));
        const uint64_t lower = heads & ((2ull << lane) - 1ull);
        head[j] = lower ? 63 - __clzll((long long)lower) : lane;
        lab[i] = counts ? (uint32_t)(ty * SPK_TW + head[j]) : SPK_NONE;
        if (lane == 0) rrow[ty] = rm[j];
    }
    __syncthreads();

    // the joins between a row and the next.  A lane whose left neighbour makes the same join on both rows has nothing
    // to add: (x, y) - (x - 1, y) - (x - 1, y + 1) - (x, y + 1) is a path already.
#pragma unroll
    for (int j = 0; j < SPK_ROWS; ++j) {
        const int ty = wave + j * SPK_WAVES, i = ty * SPK_TW + lane;
        if (!((dm[j] >> lane) & 1)) continue;
        const uint64_t covered = rm[j] & rrow[ty + 1] & dm[j];
        if (lane > 0 && ((covered >> (lane - 1)) & 1)) continue;
        lds_unite(lab, (uint32_t)(ty * SPK_TW + head[j]), lds_load(lab + i + SPK_TW));
    }
    __syncthreads();

    uint32_t root[SPK_ROWS];
#pragma unroll
    for (int j = 0; j < SPK_ROWS; ++j) {
        uint32_t r = SPK_NONE;
        if (v[j] == v[j]) {
            r = (uint32_t)((wave + j * SPK_WAVES) * SPK_TW + head[j]);
            for (uint32_t p; (p = lab[r]) < r;) r = p;
            // one LDS add per run, not per pixel: the run reaches to the first pixel that is not joined to its right
            if (head[j] == lane) atomicAdd(&cnt[r], (uint32_t)__builtin_ctzll(~rm[j] >> lane) + 1u);
        }
        root[j] = r;
    }
    __syncthreads();

#pragma unroll
    for (int j = 0; j < SPK_ROWS; ++j) {
        const int ty = wave + j * SPK_WAVES, x = x0 + lane, y = y0 + ty;
        if (x >= w || y >= h) continue;
        const size_t g = (size_t)y * w + x;
        const uint32_t r = root[j];
        label[g] = r == SPK_NONE ? SPK_NONE : (uint32_t)((size_t)(y0 + (int)(r / SPK_TW)) * w + x0 + (int)(r % SPK_TW));
        size[g] = r == (uint32_t)(ty * SPK_TW + lane) ? cnt[r] : 0;     // != 0 marks a tile-local root
    }
}

__device__ inline uint32_t agent_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a; entries only ever point at smaller indices, anything else ends the walk
__device__ inline uint32_t agent_root(const uint32_t* label, uint32_t a) {
    for (uint32_t p; (p = agent_load(label + a)) < a;) a = p;
    return a;
}

// One lane per seam pixel: first the (w - 1) / 64 vertical seams, h pixels each (the pixel left of the seam), then the
// (h - 1) / 16 horizontal ones, w pixels each (the pixel above the seam).
__global__ __launch_bounds__(256) void k_speckle_seams(const float* __restrict__ disp, uint32_t* label, int w, int h,
                                                       float vmin, float max_diff) {
    const int sx = (w - 1) / SPK_TW, sy = (h - 1) / SPK_TH;
    const long long nv = (long long)sx * h, nh = (long long)sy * w;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nv + nh) return;
    size_t p, q;
    if (t < nv) {
        const int y = (int)(t / sx), x = (int)(t % sx) * SPK_TW + SPK_TW - 1;
        p = (size_t)y * w + x;
        q = p + 1;
    } else {
        const long long u = t - nv;
        const int y = (int)(u / w) * SPK_TH + SPK_TH - 1, x = (int)(u % w);
        p = (size_t)y * w + x;
        q = p + (size_t)w;
    }
    const float a = disp[p], b = disp[q];
    if (!speckle_counts(a, vmin) || !speckle_counts(b, vmin) || !(fabsf(a - b) <= max_diff)) return;
    uint32_t ra = (uint32_t)p, rb = (uint32_t)q;
    for (;;) {
        ra = agent_root(label, ra);
        rb = agent_root(label, rb);
        if (ra == rb) return;
        if (ra < rb) { const uint32_t s = ra; ra = rb; rb = s; }
        const uint32_t old = __hip_atomic_fetch_min(label + ra, rb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old >= ra) return;
        ra = old;
    }
}

// One lane per pixel, but only a tile-local root that is no longer a root works (size[p] != 0 marks the tile-local roots):
// its count goes to the final root.  Nobody unites any more, so the roots are final; a shortened entry still points at an
// ancestor, so concurrent walks through it stay correct.
__global__ __launch_bounds__(256) void k_speckle_sum(uint32_t* label, uint32_t* size, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t l = agent_load(label + p);
    if (l >= p) return;                              // does not count, or a final root
    const uint32_t s = size[p];                      // (only a final root's entry is ever added to)
    if (s == 0) return;                              // not a tile-local root
    const uint32_t f = agent_root(label, l);
    atomicAdd(size + f, s);
    __hip_atomic_store(label + p, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// out[p] = new_val where p counts and its component has at most max_size pixels, else disp[p] (out == disp allowed:
// a lane reads and writes its own pixel only)
__global__ __launch_bounds__(256) void k_speckle_apply(const float* disp, float* out, const uint32_t* __restrict__ label,
                                                       const uint32_t* __restrict__ size, uint32_t n, uint32_t max_size,
                                                       float new_val) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    float d = disp[p];
    uint32_t r = label[p];
    if (r != SPK_NONE) {
        for (uint32_t q; r <= p && (q = label[r]) < r;) r = q;
        if (r <= p && size[r] <= max_size) d = new_val;
    }
    out[p] = d;
}

}  // namespace

size_t speckle_workspace_bytes(int w, int h) { return (size_t)w * h * 8 + 256; }

int launch_speckle_filter(int max_size, float max_diff, const float* disp, float* out, int w, int h, float vmin,
                          float new_val, void* ws, hipStream_t st) {
    const size_t n = (size_t)w * h;
    uint32_t* label = (uint32_t*)align_up((size_t)ws, 256);
    uint32_t* size = label + n;
    const unsigned tiles = (unsigned)((size_t)((w - 1) / SPK_TW + 1) * (size_t)((h - 1) / SPK_TH + 1));
    const unsigned per_pixel = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_speckle_tile, dim3(tiles), dim3(SPK_THREADS), 0, st, disp, label, size, w, h, vmin, max_diff);
    const size_t seams = (size_t)((w - 1) / SPK_TW) * h + (size_t)((h - 1) / SPK_TH) * w;
    if (seams)
        hipLaunchKernelGGL(k_speckle_seams, dim3((unsigned)((seams + 255) / 256)), dim3(256), 0, st, disp, label, w, h, vmin,
                           max_diff);
    hipLaunchKernelGGL(k_speckle_sum, dim3(per_pixel), dim3(256), 0, st, label, size, (uint32_t)n);
    hipLaunchKernelGGL(k_speckle_apply, dim3(per_pixel), dim3(256), 0, st, disp, out, label, size, (uint32_t)n,
                       (uint32_t)max_size, new_val);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

void speckle_tile(int* tw, int* th) { *tw = SPK_TW; *th = SPK_TH; }

}  // namespace smx
