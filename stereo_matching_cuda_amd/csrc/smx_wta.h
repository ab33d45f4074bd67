// smx_wta.h -- the winner-take-all pass (dispSelectOnGPU guidedFilter.cu:403-411 in packed-key form): what one pixel
// holds while a pass runs over its q values (WtaPixel: the fused aggregation's pass in smx_wta.hip and the multi-kernel
// path's k_q_wta use the same one), and the pass over materialised q planes with its one launcher.
#pragma once
#include "smx_common.h"

namespace smx {

// One pixel of a pass: the key it comes in with (or the identity), the run over this pass's ascending slices, the merge of
// the two, the stores.  NBR: the pass also keeps the winner's neighbouring q in the view's state planes nbr [3][n] (lo, hi,
// last).  The numerics are WtaRun / WtaRunNbr / nbr_prev0 / nbr_merge (smx_common.h).
// UQ: the pass also keeps the winner's second-best cost in the view's state planes uq [3][n] (sec, rest, last): WtaRunUq,
// which resumes from the stored state instead of merging, so its key is the run's own.
//   load(keys, nbr, uq, n, pix, on, fresh)   on: the pixel exists; fresh: the keys hold nothing yet -- start from the identity
//   begin(q, slice0), step(q, slice) ..      the pass's slices in ascending order, the first one through begin
//   merge(slice0)                            the run against what the pixel came in with
//   store(keys, nbr, uq, n, pix)
template <bool NBR, bool UQ = false>
struct WtaPixel;

template <>
struct WtaPixel<false, false> {
    int64_t key;
    WtaRun run;             // (the winner of this pass's slices in the float domain, packed once)
    __device__ inline void load(const int64_t* keys, const float*, const float*, size_t, size_t pix, bool on, bool fresh) {
        key = on && !fresh ? keys[pix] : KEY_IDENTITY;
    }
    __device__ inline void begin(float q, uint32_t slice0) { run.step(q, slice0); }
    __device__ inline void step(float q, uint32_t slice) { run.step(q, slice); }
    __device__ inline void merge(uint32_t) {
        const int64_t kk = run.key();
        key = kk < key ? kk : key;
    }
    __device__ inline void store(int64_t* keys, float*, float*, size_t, size_t pix) const { keys[pix] = key; }
};

template <>
struct WtaPixel<true, false> {
    int64_t key;
    float lo, hi, last, q0 = 0.0f;
    WtaRunNbr run{0.0f};
    __device__ inline void load(const int64_t* keys, const float* nbr, const float*, size_t n, size_t pix, bool on, bool fresh) {
        key = on && !fresh ? keys[pix] : KEY_IDENTITY;
        const bool ld = key != KEY_IDENTITY;            // (no winner yet: the state is not read)
        lo = ld ? nbr[pix] : 0.0f;
        hi = ld ? nbr[n + pix] : 0.0f;
        last = ld ? nbr[2 * n + pix] : 0.0f;
        run = WtaRunNbr(nbr_prev0(key, last));
    }
    __device__ inline void begin(float q, uint32_t slice0) { q0 = q; run.step(q, slice0); }     // (nbr_merge wants the first q)
    __device__ inline void step(float q, uint32_t slice) { run.step(q, slice); }
    __device__ inline void merge(uint32_t slice0) { key = nbr_merge(run, key, slice0, q0, &lo, &hi, &last); }
    __device__ inline void store(int64_t* keys, float* nbr, float*, size_t n, size_t pix) const {
        keys[pix] = key;
        nbr[pix] = lo;
        nbr[n + pix] = hi;
        nbr[2 * n + pix] = last;
    }
};

template <>
struct WtaPixel<false, true> {
    int64_t key;
    WtaRunUq run;
    __device__ inline void load(const int64_t* keys, const float*, const float* uq, size_t n, size_t pix, bool on, bool fresh) {
        key = on && !fresh ? keys[pix] : KEY_IDENTITY;
        const bool ld = key != KEY_IDENTITY;            // (no winner yet: the state is not read)
        const float sec = ld ? uq[pix] : 0.0f;
        const float rest = ld ? uq[n + pix] : 0.0f;
        const float last = ld ? uq[2 * n + pix] : 0.0f;
        run.resume(key, sec, rest, last);
    }
    __device__ inline void begin(float q, uint32_t slice0) { run.step(q, slice0); }
    __device__ inline void step(float q, uint32_t slice) { run.step(q, slice); }
    __device__ inline void merge(uint32_t) { key = run.key(); }     // (resumed from the key: nothing to merge)
    __device__ inline void store(int64_t* keys, float*, float* uq, size_t n, size_t pix) const {
        keys[pix] = key;
        uq[pix] = run.sec;
        uq[n + pix] = run.rest;
        uq[2 * n + pix] = run.last;
    }
};

// both states: the neighbour pass as it is (its merge gives the key) and the resumed uniqueness run beside it.
// Why nb.key == u.run.key() after merge, so that one store of the key serves both:
//   - nb merges the key of a run over THIS pass's slices (from m = +inf) with key_in by the integer min; u resumes (m, z*)
//     from key_in and goes on with `take = q <= m` over the same slices.  Every slice of the pass lies above z* (ascending,
//     contiguous ranges), so `q <= m` on the float side is exactly "pack_key(q, slice) < key": a smaller cost, or an equal one
//     at a larger slice; hence u ends at the integer min of key_in and the keys of all candidates, which is nb's merge
//     (test_capi.py::test_wta_run_equals_the_min_of_the_packed_keys is that statement for a single run).
//   - -0: pack_key folds it to +0 and unpack_key returns +0; -0 == +0 in every comparison, and u.key() packs once more,
//     so a winner of -0 gives the same bits either way.  A NaN is never taken by either.
//   - fresh / identity: both start blank (nb from KEY_IDENTITY, u from m = +inf, z = none); of a gated pair of passes
//     exactly one runs, and both pixels live in that one.
// tests/test_gpu_uniq.py holds the keys of every nbr+uq run to the plain call's, bit for bit.
template <>
struct WtaPixel<true, true> {
    WtaPixel<true, false> nb;
    WtaPixel<false, true> u;
    __device__ inline void load(const int64_t* keys, const float* nbr, const float* uq, size_t n, size_t pix, bool on, bool fresh) {
        nb.load(keys, nbr, nullptr, n, pix, on, fresh);
        u.load(keys, nullptr, uq, n, pix, on, fresh);
    }
    __device__ inline void begin(float q, uint32_t slice0) { nb.begin(q, slice0); u.begin(q, slice0); }
    __device__ inline void step(float q, uint32_t slice) { nb.step(q, slice); u.step(q, slice); }
    __device__ inline void merge(uint32_t slice0) { nb.merge(slice0); u.merge(slice0); }
    __device__ inline void store(int64_t* keys, float* nbr, float* uq, size_t n, size_t pix) const {
        nb.store(keys, nbr, nullptr, n, pix);   // (its key is the uniqueness run's too: WtaRunUq has WtaRun's winner)
        uq[pix] = u.run.sec;
        uq[n + pix] = u.run.rest;
        uq[2 * n + pix] = u.run.last;
    }
};

// Which pixel an element of a q plane belongs to
enum WtaOrder {
    WTA_NATURAL = 0,    // [h][w]: the ring walker's planes, the caller's volume
    WTA_COMB = 1,       // the comb walker's row-pair scratch (smx_agg_v5.h q_plane_floats, q_pixel)
};

// A pass over `count` planes (slices slice0 ..) of up to two views; keys [n] and nbr [3][n] stay in pixel order
struct WtaPass {
    const float* q[2];
    int64_t* keys[2];
    float* nbr[2];            // NULL: the plain pass
    size_t plane;             // floats from one slice's plane to the next
    size_t n;                 // pixels (w * h)
    int w, h, K;              // (K: strips of the comb scratch)
    const unsigned* gate;     // the pass runs iff gate == NULL || (*gate != 0) == gate_nonzero: which walker's planes count
    int gate_nonzero;
    int fresh;                // != 0: the keys hold nothing yet: start from the identity instead of loading them
};
// ... that also keeps the uniqueness state uq [3][n] (a type of its own: the plain and nbr kernels keep their arguments)
struct WtaPassUq : WtaPass {
    float* uq[2];
};

// The views of a pair call (smx_dev_sgm_wta_pair, _cgf_, _cross_) as its kernels index them: view k of the V given ones is the
// caller's view[k] (0 left, 1 right).  With both views the outputs hold the left view first; the one-view form has the one
// view at the front.  agg holds `count` planes a view.
struct ViewSlots {
    int V, view[2];
    int64_t* keys[2];
    float *agg[2], *nbr[2], *uq[2];
    template <class Args> void put(Args& a) const {     // into a kernel's argument struct
        for (int k = 0; k < V; ++k) { a.keys[k] = keys[k]; a.agg[k] = agg[k]; a.nbr[k] = nbr[k]; a.uq[k] = uq[k]; }
    }
};
inline ViewSlots view_slots(const float* cost_l, const float* cost_r, int64_t* keys, float* agg, float* nbr, float* uq, int count,
                            int64_t n) {
    ViewSlots s = {};
    const float* costs[2] = {cost_l, cost_r};
    for (int view = 0; view < 2; ++view) {
        if (!costs[view]) continue;
        const int64_t slot = cost_l && cost_r ? view : 0;
        s.view[s.V] = view;
        s.keys[s.V] = keys + slot * n;
        s.agg[s.V] = agg ? agg + slot * count * n : nullptr;
        s.nbr[s.V] = nbr ? nbr + slot * 3 * n : nullptr;
        s.uq[s.V] = uq ? uq + slot * 3 * n : nullptr;
        ++s.V;
    }
    return s;
}

// The one launcher: `nviews` views, q planes `plane` floats apart, nbr == NULL and uq == NULL for the plain pass, either or
// both for the passes that keep state.  Natural order takes two pixels per lane where every plane can be read in 8-byte
// units (one with nbr); comb order takes four and wants 16-byte aligned planes (SMX_E_ARG otherwise).  count < 1: no launch.
int wta_launch(WtaOrder order, int nviews, const float* const* q, int64_t* const* keys, float* const* nbr, float* const* uq,
               int w, int h, size_t plane, int count, int slice0, const unsigned* gate, int gate_nonzero, bool fresh,
               hipStream_t st);

}  // namespace smx
