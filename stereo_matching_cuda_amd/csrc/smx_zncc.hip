// ZNCC window matching cost (zero-mean normalised cross-correlation; Hirschmueller & Scharstein, PAMI 2009).  Not a stage of
// the reference: an opt-in cost that is invariant to a LOCAL affine change a*I + b, a > 0, of one image's gray values and
// keeps the magnitudes inside the window.  Contract (moments, replicate clamp, the signed square, border and flat-window
// values, slice placement): include/smx.h.
//
// k_zncc_moments: one workgroup per 64 x 8 tile of one image, as k_census: the tile plus its (rx, ry) halo is staged in LDS
// with the coordinates clamped, and a lane sums its window's values and squares from LDS.  A pixel's moments are one 8-byte
// word {S, V}.
//
// k_zncc_cost_pair: P is a box filter of the extended product row A_ext(x) * B_ext(x + d), so a cell costs O(1 + rx), not
// O(N).  A workgroup is ONE wave (its barriers cost nothing) and owns ZN_COLS = 64 - 2 * ZN_HALO columns, ZN_ROWS rows and
// ZN_Z consecutive slices of one view.  Lane t stands on the extended column x0 - ZN_HALO + t and walks down the rows with one
// running vertical sum per slice in registers: per row it adds the entering row's product and subtracts the leaving row's,
// both read from the two image tiles in LDS (rows and columns clamped when the tiles are staged, each image on its own, which
// is the definition's clamp).  A row's sums go to LDS, a lane's ZN_Z of them side by side, and the lanes of the inner columns
// add their 2 rx neighbours' in 16-byte reads, read the partner's moments (staged per row in the same phase, the variance as a
// float, a marker where the partner lies outside the image) and store one coalesced f32 per slice.  Integer sums throughout
// (bounds: include/smx.h); the f32 tail is compiled without contraction and with the correctly rounded divide, like the rest
// of this library.  Numbers and what bounds the kernel: DESIGN.md 4.3u.
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int ZM_TW = 64, ZM_TH = 8, ZM_THREADS = 256;
constexpr int ZN_R = 4;                                     // the largest radius, both ways
constexpr int ZN_THREADS = 64, ZN_HALO = ZN_R;              // one wave a workgroup: its barriers cost nothing
constexpr int ZN_COLS = ZN_THREADS - 2 * ZN_HALO;           // columns a workgroup writes
constexpr int ZN_ROWS = 32;                                 // rows a workgroup walks down
constexpr int ZN_Z = 16;                                    // slices of a workgroup
constexpr int ZN_BW = ZN_THREADS + ZN_Z;                    // partner positions of a row (one spare, keeps rows 16-byte sized)
constexpr int ZN_CS = ZN_Z / 4 + 1;                         // 16-byte words between two lanes' sums in LDS (odd: no conflicts)
constexpr uint32_t ZN_OUTSIDE = 0xBF800000u;                // -1.0f in the place of a variance: the partner lies outside the image
constexpr int ZN_TR = ZN_ROWS + 2 * ZN_R + 1;               // tile rows: the window rows of every row and the first leaving one

// grid (tiles_x * tiles_y, nimages)
__global__ __launch_bounds__(ZM_THREADS) void k_zncc_moments(const uint8_t* __restrict__ img, uint2* __restrict__ mom, int w,
                                                             int h, int rx, int ry) {
    __shared__ uint8_t tile[(ZM_TH + 2 * ZN_R) * (ZM_TW + 2 * ZN_R)];
    const int tiles_x = (w + ZM_TW - 1) / ZM_TW;
    const int x0 = (int)(blockIdx.x % tiles_x) * ZM_TW, y0 = (int)(blockIdx.x / tiles_x) * ZM_TH;
    const int64_t n = (int64_t)w * h;
    const uint8_t* I = img + (int64_t)blockIdx.y * n;
    const int hw = ZM_TW + 2 * rx, hh = ZM_TH + 2 * ry;
    for (int i = threadIdx.x; i < hw * hh; i += ZM_THREADS) {
        const int hy = i / hw, hx = i - hy * hw;
        const int y = min(max(y0 - ry + hy, 0), h - 1), x = min(max(x0 - rx + hx, 0), w - 1);
        tile[i] = I[(int64_t)y * w + x];
    }
    __syncthreads();
    const int tx = threadIdx.x & 63;
    if (x0 + tx >= w) return;
    const uint32_t N = (uint32_t)((2 * rx + 1) * (2 * ry + 1));
#pragma unroll
    for (int j = 0; j < ZM_TH / 4; ++j) {
        const int ty = (int)(threadIdx.x >> 6) + 4 * j;
        if (y0 + ty >= h) continue;
        const uint8_t* ctr = tile + (ty + ry) * hw + (tx + rx);
        uint32_t S = 0, Q = 0;
        for (int dy = -ry; dy <= ry; ++dy)
            for (int dx = -rx; dx <= rx; ++dx) {
                const uint32_t v = ctr[dy * hw + dx];
                S += v;
                Q += v * v;
            }
        mom[(int64_t)blockIdx.y * n + (int64_t)(y0 + ty) * w + (x0 + tx)] = make_uint2(S, N * Q - S * S);
    }
}

struct ZnccCostArgs {
    const uint2* mom;        // [2][h][w]: left, right
    const uint8_t* img[2];   // left, right
    float* cost[2];          // the views this launch writes (nviews of them)
    int dmin[2];
    int view[2];             // 0 left, 1 right
    int w, h, s_begin, s_end, rx, ry, xblocks;
};

// The f32 tail of a row's ZN_Z cells of one lane (include/smx.h): mb[z] is the partner's staged moments in slice z, P[z] the
// window's sum of products; out + z * n + x is the cell.  ALL: every slice is stored, else the first nz.
template <bool ALL>
__device__ __forceinline__ void zncc_finish(const int (&P)[ZN_Z], uint2 ma, const uint2* mb_row, int N, float* out, int64_t n,
                                            int x, int nz) {
    const float va = (float)ma.y;
#pragma unroll
    for (int z = 0; z < ZN_Z; ++z) {
        // The products fit 24-bit operands: N <= 81, P < 2^23, S <= 81 * 255; (float)num squared is (float)|num| squared, the
        // conversion being symmetric
        const uint2 mb = mb_row[z];
        const int num = (int)__umul24((unsigned)N, (unsigned)P[z]) - (int)__umul24(ma.x, mb.x);
        const float nf = (float)num, vb = __uint_as_float(mb.y);
        const float s = fminf((nf * nf) / (va * vb), 1.0f);
        float c = rintf(num >= 0 ? 127.5f * (1.0f - s) : 127.5f * (1.0f + s));
        c = (ma.y == 0 || vb == 0.0f) ? 128.0f : c;
        c = mb.y == ZN_OUTSIDE ? 255.0f : c;
        if (ALL || z < nz) out[(int64_t)z * n + (unsigned)x] = c;
    }
}

// grid (xblocks * yblocks, ceil(slices / ZN_Z), nviews)
__global__ __launch_bounds__(ZN_THREADS) void k_zncc_cost_pair(const ZnccCostArgs a) {
    __shared__ uint8_t tile_a[ZN_TR * ZN_THREADS];
    __shared__ uint8_t tile_b[ZN_TR * ZN_BW];
    __shared__ int4 colsum[ZN_THREADS * ZN_CS];
    __shared__ uint2 mom_b[ZN_BW];
    const int v = blockIdx.z, own = a.view[v];
    const int t = threadIdx.x, w = a.w, h = a.h, rx = a.rx, ry = a.ry;
    const int x0 = (int)(blockIdx.x % (unsigned)a.xblocks) * ZN_COLS;
    const int y0 = (int)(blockIdx.x / (unsigned)a.xblocks) * ZN_ROWS;
    const int nrows = min(ZN_ROWS, h - y0);
    const int z0 = a.s_begin + (int)blockIdx.y * ZN_Z;
    const int nz = min(ZN_Z, a.s_end - z0);
    const int64_t n = (int64_t)w * h;
    const uint8_t* A = a.img[own];
    const uint8_t* B = a.img[1 - own];
    const uint2* mom_own = a.mom + (int64_t)own * n;
    const uint2* mom_oth = a.mom + (int64_t)(1 - own) * n;
    // tile row r is image row y0 - ry - 1 + r; column j of tile_a is extended column x0 - ZN_HALO + j, column j of tile_b is
    // the partner position p0 + j, p0 = x0 - ZN_HALO + d(z0), d(z) = dmin + z.  Both clamped into their own image.
    const int64_t p0 = (int64_t)x0 - ZN_HALO + a.dmin[v] + z0;
    const int trows = nrows + 2 * ry + 1;
    for (int r = 0; r < trows; ++r) {
        const int y = min(max(y0 - ry - 1 + r, 0), h - 1), x = min(max(x0 - ZN_HALO + t, 0), w - 1);
        tile_a[r * ZN_THREADS + t] = A[(int64_t)y * w + x];
    }
    for (int i = t; i < trows * ZN_BW; i += ZN_THREADS) {
        const int r = i / ZN_BW, j = i - r * ZN_BW;
        const int y = min(max(y0 - ry - 1 + r, 0), h - 1);
        const int64_t p = p0 + j;
        const int x = (int)(p < 0 ? 0 : p > w - 1 ? w - 1 : p);
        tile_b[i] = B[(int64_t)y * w + x];
    }
    __syncthreads();
    // the window rows of row y0 but the last, and the row above them, which the first step takes out again
    int sum[ZN_Z];
#pragma unroll
    for (int z = 0; z < ZN_Z; ++z) sum[z] = 0;
    for (int r = 0; r <= 2 * ry; ++r) {
        const int av = tile_a[r * ZN_THREADS + t];
        const uint8_t* b = tile_b + r * ZN_BW + t;
#pragma unroll
        for (int z = 0; z < ZN_Z; ++z) sum[z] += av * (int)b[z];
    }
    const int x = x0 - ZN_HALO + t;
    const bool writes = t >= ZN_HALO && t < ZN_HALO + ZN_COLS && x < w;
    const int N = (2 * rx + 1) * (2 * ry + 1);
    // the partner's moments of a row: position p0 + j for j = t and, on the first ZN_Z lanes, j = ZN_THREADS + t
    const int64_t q0 = p0 + t, q1 = p0 + ZN_THREADS + t;
    const bool in0 = q0 >= 0 && q0 < w, in1 = t < ZN_Z && q1 >= 0 && q1 < w;
    for (int i = 0; i < nrows; ++i) {
        const int y = y0 + i;
        const int64_t row = (int64_t)y * w;
        // (fetched before the arithmetic that hides the latency)
        uint2 mb0 = make_uint2(0, 0), mb1 = make_uint2(0, 0), ma = make_uint2(0, 0);
        if (in0) mb0 = mom_oth[row + q0];
        if (in1) mb1 = mom_oth[row + q1];
        if (writes) ma = mom_own[row + x];
        // staged as {S, (float)V}, V < 2^31; a position outside the image holds ZN_OUTSIDE, which no variance converts to
        mb0.y = in0 ? __float_as_uint((float)mb0.y) : ZN_OUTSIDE;
        mb1.y = in1 ? __float_as_uint((float)mb1.y) : ZN_OUTSIDE;
        const int ae = tile_a[(i + 2 * ry + 1) * ZN_THREADS + t], al = tile_a[i * ZN_THREADS + t];
        const uint8_t* be = tile_b + (i + 2 * ry + 1) * ZN_BW + t;
        const uint8_t* bl = tile_b + i * ZN_BW + t;
#pragma unroll
        for (int z = 0; z < ZN_Z; ++z) sum[z] += ae * (int)be[z] - al * (int)bl[z];
        // a lane's ZN_Z sums lie together, ZN_CS 16-byte words apart from the next lane's: whole-word reads without conflicts
#pragma unroll
        for (int q = 0; q < ZN_Z / 4; ++q) colsum[t * ZN_CS + q] = make_int4(sum[4 * q], sum[4 * q + 1], sum[4 * q + 2], sum[4 * q + 3]);
        mom_b[t] = mb0;
        if (t < ZN_Z) mom_b[ZN_THREADS + t] = mb1;
        __syncthreads();
        if (writes) {
            // (ZN_HALO >= rx: the taps of a lane that writes stay inside the row)
            int P[ZN_Z];
#pragma unroll
            for (int z = 0; z < ZN_Z; ++z) P[z] = sum[z];
            for (int dx = 1; dx <= rx; ++dx) {
#pragma unroll
                for (int q = 0; q < ZN_Z / 4; ++q) {
                    const int4 lo = colsum[(t - dx) * ZN_CS + q], hi = colsum[(t + dx) * ZN_CS + q];
                    P[4 * q] += lo.x + hi.x;
                    P[4 * q + 1] += lo.y + hi.y;
                    P[4 * q + 2] += lo.z + hi.z;
                    P[4 * q + 3] += lo.w + hi.w;
                }
            }
            float* out = a.cost[v] + ((int64_t)(z0 - a.s_begin) * n + row);      // (the same for every lane)
            // (a workgroup with all its slices stores without a test per slice: one block of code, its LDS reads up front)
            if (nz == ZN_Z) zncc_finish<true>(P, ma, mom_b + t, N, out, n, x, nz);
            else zncc_finish<false>(P, ma, mom_b + t, N, out, n, x, nz);
        }
        __syncthreads();
    }
}

}  // namespace

void zncc_geometry(int* cols, int* rows) {
    *cols = ZN_COLS;
    *rows = ZN_ROWS;
}

int launch_zncc_moments(int rx, int ry, const uint8_t* img, uint64_t* mom, int w, int h, int nimages, hipStream_t st) {
    const long long tiles = (long long)((w + ZM_TW - 1) / ZM_TW) * ((h + ZM_TH - 1) / ZM_TH);
    if (tiles > 0x7FFFFFFFll || nimages > 65535)
        return fail(SMX_E_ARG, "smx_dev_zncc_moments: %d images of %d x %d are too many tiles", nimages, w, h);
    hipLaunchKernelGGL(k_zncc_moments, dim3((unsigned)tiles, (unsigned)nimages), dim3(ZM_THREADS), 0, st, img, (uint2*)mom, w, h,
                       rx, ry);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

int launch_zncc_cost_pair(int rx, int ry, const uint64_t* mom, const uint8_t* img_l, const uint8_t* img_r, float* cost_l,
                          float* cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end, hipStream_t st) {
    if (s_end <= s_begin) return SMX_OK;
    ZnccCostArgs a;
    a.mom = (const uint2*)mom;
    a.img[0] = img_l; a.img[1] = img_r;
    int nviews = 0;
    if (cost_l) { a.cost[nviews] = cost_l; a.dmin[nviews] = dminl; a.view[nviews] = 0; ++nviews; }
    if (cost_r) { a.cost[nviews] = cost_r; a.dmin[nviews] = dminr; a.view[nviews] = 1; ++nviews; }
    for (int v = nviews; v < 2; ++v) { a.cost[v] = nullptr; a.dmin[v] = 0; a.view[v] = 0; }
    a.w = w; a.h = h; a.s_begin = s_begin; a.s_end = s_end; a.rx = rx; a.ry = ry;
    a.xblocks = (w + ZN_COLS - 1) / ZN_COLS;
    const long long groups = (long long)a.xblocks * ((h + ZN_ROWS - 1) / ZN_ROWS);
    const long long zblocks = ((long long)s_end - s_begin + ZN_Z - 1) / ZN_Z;
    if (groups > 0x7FFFFFFFll || zblocks > 65535)
        return fail(SMX_E_ARG, "smx_dev_zncc_cost_pair: %d x %d with %d slices is too many workgroups", w, h, s_end - s_begin);
    hipLaunchKernelGGL(k_zncc_cost_pair, dim3((unsigned)groups, (unsigned)zblocks, (unsigned)nviews), dim3(ZN_THREADS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
