// AD-Census matching cost (Mei et al. 2011): the census / Hamming cost of smx_census.hip plus the absolute difference of the
// pixels, each through rho(c, lambda) = 1 - exp(-c / lambda) and added.  Not a stage of the reference: an opt-in cost for
// the case the census cost cannot decide -- patches of equal local ORDER and different magnitudes cost 0 against each other.
// Contract (tables, border cost, slice placement): include/smx.h.  rho comes from a table the host computes in double
// (smx_adcensus_tables), so the kernel holds no transcendental and the volume equals tests/adcensus_ref.py bit for bit.
//
// k_adcensus_cost_pair: the decomposition of k_census_cost_pair, a pure store stream (2 * slices * w * h floats).  A
// workgroup owns 256 columns of one row of one view and AC_Z consecutive slices.  Staged in LDS once: the 256 + AC_Z - 1
// codes of the other view those slices touch (positions outside the image hold a marker with bit 63 set, which no code
// has), the pixels at the same positions as one 32-bit word each (gray in byte 0, or R, G, B in bytes 0 .. 2; byte 3 is 0,
// so 3- and 4-channel images meet in one inner loop), and the part of the table the call can index.  A lane keeps its own
// code and pixel word in three VGPRs and does, per slice: one 8-byte and one 4-byte LDS read, two xor, two popcounts, a min,
// one packed sum of absolute differences (v_sad_u8), two table reads, one add, a select and one coalesced 4-byte store.
// Plain stores, as in the census kernel.
#include "smx_launch.h"

namespace smx {
namespace {

constexpr int AC_COLS = 256;                                // columns (= lanes) of a cost workgroup
constexpr int AC_Z = 16;                                    // slices of a cost workgroup
constexpr uint64_t AC_OUTSIDE = 0x8000000000000000ull;      // the partner lies outside the image
constexpr int AC_CENSUS = 64;                               // T[0 .. 63]: the census half; T[64 + s]: the AD half

struct AdCensusArgs {
    const float* table;      // SMX_ADCENSUS_TABLE_FLOATS
    const uint64_t* code;    // [2][h][w]: left, right
    const uint8_t* img[2];   // [h][w][ch]: left, right
    float* cost[2];          // the views this launch writes (nviews of them)
    int dmin[2];
    int view[2];             // 0 left, 1 right
    int w, h, s_begin, s_end, t, xblocks;
    int ch;                  // bytes per pixel: 1 (gray), 3 or 4 (R, G, B first)
    int ntab;                // table entries the call can index: 64 + 255 * nch + 1
};

// the pixel at `q` as the word the inner loop compares: gray, or R | G << 8 | B << 16
__device__ __forceinline__ uint32_t ac_pixel(const uint8_t* q, int ch) {
    uint32_t v = q[0];
    if (ch != 1) v |= (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
    return v;
}

// grid (xblocks * h, ceil(slices / AC_Z), nviews)
__global__ __launch_bounds__(AC_COLS) void k_adcensus_cost_pair(const AdCensusArgs a) {
    __shared__ uint64_t other[AC_COLS + AC_Z - 1];
    __shared__ uint32_t opix[AC_COLS + AC_Z - 1];
    __shared__ float tab[SMX_ADCENSUS_TABLE_FLOATS];
    const int v = blockIdx.z;
    const int y = (int)(blockIdx.x / (unsigned)a.xblocks);
    const int x0 = (int)(blockIdx.x % (unsigned)a.xblocks) * AC_COLS;
    const int z0 = a.s_begin + (int)blockIdx.y * AC_Z;
    const int nz = min(AC_Z, a.s_end - z0);
    const int ch = a.ch;
    const int64_t n = (int64_t)a.w * a.h, row = (int64_t)y * a.w;
    const uint64_t* own_codes = a.code + (int64_t)a.view[v] * n + row;
    const uint64_t* oth_codes = a.code + (int64_t)(1 - a.view[v]) * n + row;
    const uint8_t* own_img = a.img[a.view[v]] + row * ch;
    const uint8_t* oth_img = a.img[1 - a.view[v]] + row * ch;
    for (int i = threadIdx.x; i < a.ntab; i += AC_COLS) tab[i] = a.table[i];
    // other[j] / opix[j] = the other view's code / pixel at x0 + d(z0) + j, d(z) = dmin + z
    const int64_t p0 = (int64_t)x0 + a.dmin[v] + z0;
    for (int j = threadIdx.x; j < AC_COLS + nz - 1; j += AC_COLS) {
        const int64_t p = p0 + j;
        const bool in = p >= 0 && p < a.w;
        other[j] = in ? oth_codes[p] : AC_OUTSIDE;
        opix[j] = in ? ac_pixel(oth_img + p * ch, ch) : 0u;
    }
    __syncthreads();
    const int x = x0 + (int)threadIdx.x;
    if (x >= a.w) return;
    const uint64_t own = own_codes[x];
    const uint32_t pix = ac_pixel(own_img + (int64_t)x * ch, ch);
    const uint32_t t = (uint32_t)a.t;
    const float border = tab[t] + tab[a.ntab - 1];          // T[t] + T[64 + 255 nch]
    float* out = a.cost[v] + (int64_t)(z0 - a.s_begin) * n + row + x;
#pragma unroll 4
    for (int z = 0; z < nz; ++z) {
        const uint64_t d = own ^ other[threadIdx.x + z];
        const uint32_t hc = min((uint32_t)__popcll(d), t);   // (a marker's popcount is not used: the select below)
        const uint32_t s = __builtin_amdgcn_sad_u8(pix, opix[threadIdx.x + z], 0u);
        const float c = tab[hc] + tab[AC_CENSUS + s];
        out[(int64_t)z * n] = (int64_t)d < 0 ? border : c;
    }
}

}  // namespace

int launch_adcensus_cost_pair(int t, int nch, const float* table, const uint64_t* code, const uint8_t* img_l, const uint8_t* img_r,
                              int ch, float* cost_l, float* cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end,
                              hipStream_t st) {
    if (s_end <= s_begin) return SMX_OK;
    AdCensusArgs a;
    a.table = table;
    a.code = code;
    a.img[0] = img_l; a.img[1] = img_r;
    int nviews = 0;
    if (cost_l) { a.cost[nviews] = cost_l; a.dmin[nviews] = dminl; a.view[nviews] = 0; ++nviews; }
    if (cost_r) { a.cost[nviews] = cost_r; a.dmin[nviews] = dminr; a.view[nviews] = 1; ++nviews; }
    for (int v = nviews; v < 2; ++v) { a.cost[v] = nullptr; a.dmin[v] = 0; a.view[v] = 0; }
    a.w = w; a.h = h; a.s_begin = s_begin; a.s_end = s_end; a.t = t;
    a.ch = ch;
    a.ntab = AC_CENSUS + 255 * nch + 1;
    a.xblocks = (w + AC_COLS - 1) / AC_COLS;
    const long long rows = (long long)a.xblocks * h;
    const long long zblocks = ((long long)s_end - s_begin + AC_Z - 1) / AC_Z;
    if (rows > 0x7FFFFFFFll || zblocks > 65535)
        return fail(SMX_E_ARG, "smx_dev_adcensus_cost_pair: %d x %d with %d slices is too many workgroups", w, h, s_end - s_begin);
    hipLaunchKernelGGL(k_adcensus_cost_pair, dim3((unsigned)rows, (unsigned)zblocks, (unsigned)nviews), dim3(AC_COLS), 0, st, a);
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
