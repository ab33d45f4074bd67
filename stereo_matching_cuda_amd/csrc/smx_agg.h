// smx_agg.h -- the aggregation as the C-ABI sees it (smx_agg.hip): the description of a call, which aggregation it runs, the
// one description of each workspace, the orchestration of the two walkers (comb: smx_agg_v5.hip, ring: smx_agg_v4.hip) and of
// the multi-kernel path (smx_kernels.hip).
#pragma once
#include "smx_common.h"

namespace smx {

// One aggregation call: aggregation + WTA of slices [s_begin, s_end) of `nviews` (1 or 2) views.  View v uses guide[v] as
// guidance; its cost slices are cost[v] (materialised, slice s at (s - s_begin)*w*h; all views or none) or, where cost[v] is
// NULL, are built on the fly against other[v].  Pointers are NULL where absent: mean_u8 (the u8 mean image), agg (the
// aggregated volume), nbr (the winners' neighbours, smx_common.h nbr_merge), uq (the winners' second-best cost, smx_common.h
// WtaRunUq).  Everything a call depends on is here or in AggOpts.
struct AggCall {
    const char* who;         // the C-ABI entry, for error texts
    const smx_params* p;
    int nviews;
    const uint8_t* guide[2];
    const uint8_t* other[2];
    const float* cost[2];
    int dmin[2];             // disparity of slice 0
    int64_t* keys[2];        // IN/OUT: the packed WTA keys [h][w]
    uint8_t* mean_u8[2];
    float* agg[2];
    float* nbr[2];
    float* uq[2];
    int w, h, s_begin, s_end;
    void* ws;                // the caller's workspace, any alignment
    size_t ws_bytes;
    hipStream_t st;
};
// Options / report of one call (set and read through the C-ABI: smx_set_max_slices_per_launch, smx_set_keys_fresh,
// smx_last_agg_path, smx_last_agg_chunk, smx_last_agg_ms)
struct AggOpts {
    bool fast = false;       // FAST mode (not bit-exact)
    int walker = 0;          // 0 choose, 4 ring walker forced, 5 comb walker forced (an error where it does not apply)
    int max_chunk = 0;       // upper bound on the slices of one walker launch; 0 = as many as the workspace holds
    bool keys_fresh = false; // the keys hold nothing yet: the first WTA pass starts from the identity (no smx_dev_init_keys needed)
    // fast / walker of a fused path agg_path_for chose (2, 4, 5); `aggregate` sets them itself
    void take_path(int path) { fast = path == 4; walker = path == 2 ? 4 : path == 5 ? 5 : 0; }
};
struct AggInfo {
    int path = 0;            // the aggregation that ran: 1 multi-kernel, 2 ring walker, 4 FAST, 5 comb walker
    int walker_used = 0;     // 4 ring walker, 5 comb walker; 0 on the multi-kernel path
    int chunk = 0;           // slices per walker launch (of the first = largest launch) / per pass of the multi-kernel path
    int walker_launches = 0;
    int launches = 0;        // all kernel launches + memsets of the call
};

// The one decision of which aggregation a call runs (smx_dev_aggregate_wta, the pair entries, the context, the workspace size):
// 1 the multi-kernel path, 2 the ring walker, 4 FAST, 5 the comb walker; 0, with *why set, where the forced path does not apply.
// forced is the caller's smx_set_agg_path value: 0 auto, 1 multi-kernel, 2 fused (walker chosen here), 3 ring walker, 4 FAST,
// 5 comb walker.  Pure host arithmetic (no GPU needed: smx_debug_agg_path).
int agg_path_for(const smx_params* p, int w, int h, int nviews, bool use_cost, int forced, const char** why);

// The workspace of one fused aggregation call.  Byte offsets from the 256-byte aligned start of the caller's workspace, in
// carving order; every region is a multiple of 256 bytes.  All sizes derive from this: the carving of aggregate_fused, the
// comb walker's descriptor bound (v5_fix_bytes), the chunk a workspace holds (agg_plan) and agg_workspace_bytes.
struct AggLayout {
    bool comb;            // the comb walker runs (else the ring walker)
    bool fallback;        // ... with the ring walker queued behind it (materialised cost volumes)
    bool own_q;           // the q planes live here (else the walkers write the caller's volume)
    int nviews, chunk;    // views, slices per walker launch
    int K, NI;            // strips and bands of the walker that runs
    int K4, NI4;          // the ring walker's (what a queued fall-back runs with)
    int K_flags;          // flag words per slice-view (fall-back: the larger of the two walkers')
    size_t plane;         // floats per [h][w] plane
    size_t qplane;        // floats per slice of q (own planes of the comb walker are comb-ordered: K * OWS >= w columns per row)
    size_t q_slice;       // bytes per slice of a view's own q planes; 0: the caller's volume
    size_t hand_sv;       // floats of hand-off records per slice-view (fall-back: the larger of the two walkers')
    // ---- the fixed part
    size_t status;        // 256 B: the call's status words (smx_dev_agg_status, smx_dev_agg_fallback)
    size_t fg[2];         // both image planes [h][w + 2 PADX] (a single view's partner too)
    size_t guid[2];       // per view: (mean_I, 1/(var_I + eps)) [h][w]
    size_t g1p[2], i2p[2];   // per view, comb walker only: the comb-ordered copies (smx_agg_v5.h), view by view
    size_t fix_end;       // [fg[0], fix_end): what the comb walker addresses through its one 32-bit-offset descriptor
    size_t scratch[2][2]; // per view: integrals of I and of I*I
    size_t chunk_begin;   // ---- per chunk of `chunk` slices
    size_t q[2];          // per view: own q planes, q_slice apart
    size_t hand;          // hand-off records of chunk * nviews slice-views
    size_t ctrl;          // control block: ticket (AGG_CTRL_BYTES) + flags [sv][K_flags]
    size_t ctrl_bytes;
    size_t end;
};
constexpr size_t AGG_CTRL_BYTES = 256;   // ticket (zeroed with the flags before every launch)
AggLayout agg_layout(int w, int h, int radius, int nviews, bool comb, bool fallback, bool own_q, int chunk);
// The layout a call runs with -- walker, queued fall-back, the chunk its workspace holds (at most `total` slices and
// opt.max_chunk) -- or the call's error.  `lost`: the bytes in front of the workspace's 256-byte boundary.  Pure host
// arithmetic (smx_debug_agg_chunk).
int agg_plan(const smx_params* p, int w, int h, int nviews, bool use_cost, bool own_q, const AggOpts& opt, size_t ws_bytes,
             size_t lost, int total, AggLayout* L);
// bytes for ONE view with `nslices` slices in flight, whichever walker and radius the call runs (q planes included)
size_t agg_workspace_bytes(int w, int h, int nslices);
// Bytes of the region the comb walker addresses through its one 32-bit-offset descriptor
size_t v5_fix_bytes(int w, int h, int nviews);
// status words of the last fused aggregation that used this workspace: [0] != 0: a hand-off wait timed out;
// [1] != 0: the comb walker met cost values outside its exactness argument and the queued ring walker redid the chunk
int agg_read_status(const void* d_ws, unsigned* out, int nwords);

// The workspace of one call on the multi-kernel path, in the same terms.  The views of a call run one after the other in the
// same planes.  The volumes of a chunk are packed with a plane stride of w*h floats (the kernels index planes as z*w*h).
struct MultiLayout {
    int chunk;            // slices per pass
    int volumes;          // volumes of a chunk: T0, T1, A, B and, where the costs are built from the images, C
    size_t status;        // 256 B: the status words (smx_dev_agg_status; this path cannot time out: cleared, never raised)
    size_t im, mean_im, cinv, g0, g1;   // [h][w] f32 each: the image, mean_I, 1/(var_I + eps), two integrals
    size_t chunk_begin;   // ---- per chunk of `chunk` slices, [chunk][h][w] f32 each
    size_t T0, T1, A, B;
    size_t C;             // the costs, where they are built from the images (else 0: none)
    size_t end;
};
MultiLayout multi_layout(int w, int h, bool use_cost, int chunk);
// The layout a call runs with -- the chunk its workspace holds, at most `total` slices; opt.max_chunk is "of the fused
// aggregation" (smx.h) and not honoured -- or SMX_E_WS in the name of `who`.  Pure host arithmetic (smx_debug_agg_chunk).
int multi_plan(const char* who, int w, int h, bool use_cost, size_t ws_bytes, size_t lost, int total, MultiLayout* L);
// bytes for ONE view with `nslices` slices in flight on the multi-kernel path
size_t multi_workspace_bytes(int w, int h, int nslices);

// The one way into an aggregation: decides the path (agg_path_for with the caller's `forced`; an error in the name of c.who
// where it does not apply) and runs the fused aggregation or the multi-kernel path for all views of the call.  opt: max_chunk
// and keys_fresh; fast / walker follow from the path.
int aggregate(const AggCall& c, int forced, const AggOpts& opt, AggInfo* info);

}  // namespace smx
