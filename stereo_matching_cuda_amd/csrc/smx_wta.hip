// smx_wta.hip -- the WTA pass of the fused aggregation over the chunk's materialised q planes (smx_wta.h): ONE kernel
// body for every layout the walkers leave q in.  What differs between the forms is which pixel an element of a plane belongs
// to (Order), how many consecutive elements a lane takes (EPL: 4-, 8- or 16-byte loads) and which state is kept beside
// the keys: the winner's neighbours (NBR), its second-best cost (UQ), both or none.
//
// Must be compiled with -ffp-contract=off.
#include "smx_wta.h"

#include <type_traits>

#include "smx_agg_dev.h"
#include "smx_agg_v5.h"

namespace smx {
using namespace aggdev;

// ---- orders: elements(a) = elements of a plane that lanes are dealt; pixel(a, e, &pix) = the pixel of element e, false where
// the element belongs to none.  A lane's EPL elements start at a multiple of EPL.
struct Natural {    // [h][w]: pixel = element.  (two per lane only where n is even -- wta_launch: a lane's elements exist together)
    __device__ static inline size_t elements(const WtaPass& a) { return a.n; }
    __device__ static inline bool pixel(const WtaPass&, size_t e, size_t* pix) { *pix = e; return true; }
};
struct Comb {       // [K][ceil(h/2)][OWS][2] (smx_agg_v5.h): a plane is a whole number of quads, so is a.plane
    __device__ static inline size_t elements(const WtaPass& a) { return a.plane; }
    __device__ static inline bool pixel(const WtaPass& a, size_t e, size_t* pix) {
        int x, y;
        const bool in = v5::q_pixel(e, a.w, a.h, a.K, &x, &y);
        *pix = in ? (size_t)y * a.w + x : 0;
        return in;
    }
};

// One lane = EPL consecutive elements of every plane, coalesced nt loads, eight planes in flight; keys and neighbour state stay
// in pixel order -- the lane finds its pixels once per call.  grid (ceil(elements / (256 EPL)), nviews)
template <bool UQ> using PassOf = std::conditional_t<UQ, WtaPassUq, WtaPass>;
__device__ inline float* uq_of(const WtaPass&, int) { return nullptr; }
__device__ inline float* uq_of(const WtaPassUq& a, int v) { return a.uq[v]; }

template <class Order, int EPL, bool NBR, bool UQ>
__global__ __launch_bounds__(256) void k_wta(PassOf<UQ> a, int count, int slice0) {
    typedef float fv __attribute__((ext_vector_type(EPL)));
    const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * EPL;
    // (the gate is uniform: every thread reads the same word)
    if (e0 >= Order::elements(a) || (a.gate && (int)(flag_load(const_cast<unsigned*>(a.gate)) != 0u) != a.gate_nonzero)) return;
    const float* __restrict__ q = a.q[blockIdx.y] + e0;
    int64_t* const keys = a.keys[blockIdx.y];
    float* const nbr = a.nbr[blockIdx.y];
    float* const uq = uq_of(a, blockIdx.y);
    size_t pix[EPL];
    bool in[EPL];
    WtaPixel<NBR, UQ> px[EPL];
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        in[j] = Order::pixel(a, e0 + j, &pix[j]);
        px[j].load(keys, nbr, uq, a.n, pix[j], in[j], a.fresh != 0);
    }
    // nothing of this lane lies in the image (the tail of a row of the comb scratch's last strip): no load at all
    bool any = false;
#pragma unroll
    for (int j = 0; j < EPL; ++j) any = any || in[j];
    if (!any) return;
    auto plane = [&](int z) { return __builtin_nontemporal_load((const fv*)&q[(size_t)z * a.plane]); };
    int z = 0;
    if constexpr (NBR) {        // (the neighbour merge wants the pass's first q by itself)
        const fv v = plane(0);
#pragma unroll
        for (int j = 0; j < EPL; ++j) px[j].begin(v[j], (uint32_t)slice0);
        z = 1;
    }
    constexpr int U = 8;        // loads in flight per lane (4 / 16 / 24 measure the same)
    for (; z + U <= count; z += U) {
        fv v[U];
#pragma unroll
        for (int t = 0; t < U; ++t) v[t] = plane(z + t);
#pragma unroll
        for (int t = 0; t < U; ++t)
#pragma unroll
            for (int j = 0; j < EPL; ++j) px[j].step(v[t][j], (uint32_t)(slice0 + z + t));
    }
    for (; z < count; ++z) {
        const fv v = plane(z);
#pragma unroll
        for (int j = 0; j < EPL; ++j) px[j].step(v[j], (uint32_t)(slice0 + z));
    }
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
        px[j].merge((uint32_t)slice0);
        if (in[j]) px[j].store(keys, nbr, uq, a.n, pix[j]);
    }
}

template <class Order, int EPL, bool NBR, bool UQ>
static void launch(const PassOf<UQ>& a, size_t elements, int nviews, int count, int slice0, hipStream_t st) {
    const size_t per_wg = (size_t)256 * EPL;
    hipLaunchKernelGGL((k_wta<Order, EPL, NBR, UQ>), dim3((unsigned)((elements + per_wg - 1) / per_wg), (unsigned)nviews), dim3(256),
                       0, st, a, count, slice0);
}

int wta_launch(WtaOrder order, int nviews, const float* const* q, int64_t* const* keys, float* const* nbr, float* const* uq,
               int w, int h, size_t plane, int count, int slice0, const unsigned* gate, int gate_nonzero, bool fresh,
               hipStream_t st) {
    WtaPassUq a;
    for (int v = 0; v < 2; ++v) {
        const int vv = v < nviews ? v : 0;
        a.q[v] = q[vv]; a.keys[v] = keys[vv]; a.nbr[v] = nbr ? nbr[vv] : nullptr; a.uq[v] = uq ? uq[vv] : nullptr;
    }
    a.plane = plane;
    a.n = (size_t)w * h;
    a.w = w; a.h = h; a.K = v5::strips(w);
    a.gate = gate; a.gate_nonzero = gate_nonzero;
    a.fresh = fresh ? 1 : 0;
    // (every element a lane touches lies inside its plane: the comb decode is that of exactly this plane size)
    if (order == WTA_COMB ? plane != v5::q_plane_floats(w, h) : plane < a.n) return fail(SMX_E_ARG, "wta_launch: plane stride");
    if (order == WTA_COMB) {
        for (int v = 0; v < nviews; ++v)
            if (((uintptr_t)a.q[v] & 15) != 0) return fail(SMX_E_ARG, "wta_launch: q scratch of view %d is not 16-byte aligned", v);
    }
    if (count < 1) return SMX_OK;
    if (order == WTA_COMB) {
        if (nbr && uq) launch<Comb, 4, true, true>(a, plane, nviews, count, slice0, st);
        else if (uq) launch<Comb, 4, false, true>(a, plane, nviews, count, slice0, st);
        else if (nbr) launch<Comb, 4, true, false>(a, plane, nviews, count, slice0, st);
        else launch<Comb, 4, false, false>(a, plane, nviews, count, slice0, st);
    } else {
        // two pixels per lane where every plane can be read in 8-byte units
        bool al8 = a.n % 2 == 0 && plane % 2 == 0;
        for (int v = 0; v < nviews; ++v) al8 = al8 && ((uintptr_t)a.q[v] & 7) == 0;
        if (nbr && uq) launch<Natural, 1, true, true>(a, a.n, nviews, count, slice0, st);
        else if (uq && al8) launch<Natural, 2, false, true>(a, a.n, nviews, count, slice0, st);
        else if (uq) launch<Natural, 1, false, true>(a, a.n, nviews, count, slice0, st);
        else if (nbr) launch<Natural, 1, true, false>(a, a.n, nviews, count, slice0, st);
        else if (al8) launch<Natural, 2, false, false>(a, a.n, nviews, count, slice0, st);
        else launch<Natural, 1, false, false>(a, a.n, nviews, count, slice0, st);
    }
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

}  // namespace smx
