// smx_ctx.hip -- the persistent context of the host-pointer pair entry (smx_create .. smx_ctx_wait, smx_stereo_pair).  What a
// pair runs, needs and refuses is decided once by plan_pair (smx_ctx_plan.h: the settings, the stage table, the PairPlan), before
// anything is allocated; the plan is reserved in one place (ctx_reserve) and run by ctx_enqueue, which both entries share.
// A new opt-in stage takes a row of that table, its buffers in ctx_reserve, its launch in ctx_enqueue and its setter here.
#include <string.h>

#include <array>
#include <new>
#include <vector>

#include "smx_api.h"
#include "smx_launch.h"

using namespace smx;

struct smx_ctx {
    smx_params p;
    int w = 0, h = 0, size_d = 0, dev = -1;
    int agg_path = 0;      // this context's aggregation path (smx_ctx_set_agg_path); starts as the creating thread's
    size_t n = 0, ws_bytes = 0;
    hipStream_t st = nullptr;
    // keys / best / dmap / mean: left view first, right view behind it (one buffer each)
    DevBuf dL, dR, keys, best, map, mean, occ, fil, ws, costL, costR, aggLR;
    // The opt-in stages: their settings, the plan of the last synchronous pair that completed (all false while none has: the
    // smx_ctx_*_map(s) getters read it), and their buffers, allocated on first use (ctx_reserve).
    CtxSettings s;
    PairPlan done;
    DevBuf nbr, sub, subf;      // sub-pixel: neighbour state [2][3][h][w], maps [2][h][w] and [h][w]
    DevBuf codes;               // census cost, AD-Census: the codes [2][h][w]; the ZNCC cost: the moments [2][h][w], as large
    bool adc_tab_valid = false; // the device table holds the tables of s.adc
    DevBuf adc_tab;
    // the mutual-information cost: the histogram [256][256] u32 and the table [256][256] u8 of the pass in hand; mi_table is
    // what the cost kernel reads -- this context's table, or in a pyramid level the table of level 0
    DevBuf mi_hist, mi_tab;
    const uint8_t* mi_table = nullptr;
    bool done_mi = false;       // the last synchronous pair that completed ran with it (smx_ctx_mi_table)
    DevBuf spk, spk_ws;         // speckle removal: the despeckled left map [h][w] and the filter's workspace
    DevBuf uq, uq_map, uq_margin;   // uniqueness: the state [2][3][h][w], the filtered left map and the margins [h][w]
    DevBuf rgb;                 // the two colour images [2][h][w][4]
    // the scan-line optimiser: its workspace and, behind cross-based aggregation, the two volumes of q [2][size_d][h][w]
    DevBuf so_ws, so_vol;
    DevBuf varms, voted, vote_ws;   // region voting: the arms of the left guide [h][w], the voted left map [h][w], the workspace
    DevBuf adj_ws;              // the adjustment's workspace; it reads the left volume of aggLR
    // cross-scale aggregation: a child context per level 1 .. scales-1, created on first use at the level's geometry, on this
    // context's stream (owns_st false: the stream is the parent's).  A child holds its level's images (dL, dR, rgb) and
    // aggregated volumes (aggLR), and is made anew where a pair's label ranges ask for another size_d
    smx_ctx* cs_child[SMX_CSCALE_MAX_SCALES] = {};
    bool owns_st = true;
    // PatchMatch stereo: the planes [2][3][h][w], disp [2][h][w] and the search's workspace; its sub-pixel filled map lies in subf
    DevBuf pm_planes, pm_disp, pm_ws;
    DevBuf perm_ws;             // the permeability filter runs in place over both volumes of aggLR; its workspace
    // the tree filter, the second mode of the permeability filter's place: its workspace, the two blobs [2][smx_tree_bytes] on
    // the device and, on the host, the blobs as they are built and the gray guides of a colour pair under the gray guide
    DevBuf tree_ws, tree_dev;
    std::vector<uint32_t> tree_host;
    std::vector<uint8_t> tree_gray;
    DevBuf bp_ws;               // belief propagation reads the whole volumes costL / costR, as SGM does; its workspace
    // What the pair in hand takes of the buffers that the opt-in flows share (ctx_reserve sets them per pair).  mode_ws: the
    // workspace for both views of SGM, the colour-guided filter or cross-based aggregation -- a pair runs at most one of them --
    // of which this pair's mode and chunk use mode_ws_bytes; the buffer itself only grows, so it may be larger.  chunk: the
    // slices ctx_aggregate_chunks takes at a time; chunk_cost: without whole volumes, one chunk of both views' cost slices
    // [2][chunk][h][w].
    int chunk = 0;
    size_t mode_ws_bytes = 0;
    DevBuf mode_ws, chunk_cost;
    // pipelined entry: two slots of device inputs / results and pinned staging, created on first use.  Staging of a slot:
    // [gray_l | gray_r] going up; [best_l best_r dmap_l dmap_r occlusion filled | mean_l mean_r | status word] coming down.
    struct Slot {
        DevBuf in, res, mean;
        uint8_t* h_in = nullptr;
        char* h_out = nullptr;
        hipEvent_t up = nullptr, done = nullptr, down = nullptr;
    } slot[2];
    hipStream_t st_up = nullptr, st_dn = nullptr;
    uint64_t submitted = 0, waited = 0;
    ~smx_ctx() {
        for (smx_ctx* k : cs_child) delete k;
        if (!owns_st) st = nullptr;
        for (Slot& sl : slot) {
            if (sl.h_in) (void)hipHostFree(sl.h_in);
            if (sl.h_out) (void)hipHostFree(sl.h_out);
            for (hipEvent_t e : {sl.up, sl.done, sl.down})
                if (e) (void)hipEventDestroy(e);
        }
        for (hipStream_t x : {st, st_up, st_dn})
            if (x) (void)hipStreamDestroy(x);
    }
};

// The permeability filter's workspace for both views: every slice at once where that stays within ~1 GiB, else what does, and one
// slice at least (the pass goes in chunks of slices over the volumes it filters in place)
static size_t ctx_perm_ws_bytes(const smx_ctx* c) {
    const size_t cap = (size_t)1 << 30, per = 2 * c->n * sizeof(float);
    size_t k = cap / per > 2 ? cap / per - 2 : 1;
    if (k > (size_t)c->size_d) k = (size_t)c->size_d;
    return per * (2 + k);
}
// The tree filter's workspace for both views under the same rule: a breadth-first plane per view and slice in flight
static size_t ctx_tree_ws_bytes(const smx_ctx* c) {
    const size_t cap = (size_t)1 << 30, per = 2 * c->n * sizeof(float);
    size_t k = cap / per > 1 ? cap / per : 1;
    if (k > (size_t)c->size_d) k = (size_t)c->size_d;
    return per * k;
}
struct PairIn { const uint8_t* left; const uint8_t* right; int dminl, dminr; const uint8_t* rgb_l; const uint8_t* rgb_r; int channels; };
struct PairPlanes { float* best; float* map; uint8_t* mean; float* occ; float* fil; };

// The most slices in flight whose workspace for both views -- and chunk of cost slices, without whole volumes -- stay within
// ~2 GiB, by halving
static int halved_chunk(const smx_ctx* c, size_t (*ws_bytes)(int, int, int, int), bool whole) {
    const size_t cap = (size_t)2 << 30, fb = c->n * sizeof(float);
    int k = c->size_d;
    while (k > 1 && ws_bytes(c->w, c->h, k, 2) + (whole ? 0 : 2 * (size_t)k * fb) > cap) k = (k + 1) / 2;
    return k;
}

// Every buffer `need` asks for, each under its own guard: after a failed allocation the next call simply retries.
static int ctx_reserve(smx_ctx* c, const PairPlan& need) {
    const size_t fb = c->n * sizeof(float), vb = fb * c->size_d;
    if (need.cost) { SMX_HIP(c->costL.ensure(vb)); SMX_HIP(c->costR.ensure(vb)); }
    if (need.agg) SMX_HIP(c->aggLR.ensure(2 * vb));
    if (need.subpix) { SMX_HIP(c->nbr.ensure(6 * fb)); SMX_HIP(c->sub.ensure(2 * fb)); SMX_HIP(c->subf.ensure(fb)); }
    const bool mi = c->s.cost_mode == SMX_COST_MI;
    if (need.census && !mi) SMX_HIP(c->codes.ensure(2 * c->n * sizeof(uint64_t)));
    if (need.census && mi && !need.level) {
        SMX_HIP(c->mi_hist.ensure((size_t)SMX_MI_LEVELS * SMX_MI_LEVELS * sizeof(uint32_t)));
        SMX_HIP(c->mi_tab.ensure((size_t)SMX_MI_LEVELS * SMX_MI_LEVELS));
        c->mi_table = c->mi_tab.as<uint8_t>();
    }
    if (need.speckle) { SMX_HIP(c->spk.ensure(fb)); SMX_HIP(c->spk_ws.ensure(speckle_workspace_bytes(c->w, c->h))); }
    if (need.uniq) { SMX_HIP(c->uq.ensure(6 * fb)); SMX_HIP(c->uq_map.ensure(fb)); SMX_HIP(c->uq_margin.ensure(fb)); }
    if (need.so) {
        SMX_HIP(c->so_ws.ensure(scanline_workspace_bytes(c->w, c->h, c->size_d, 2)));
        if (need.cross) SMX_HIP(c->so_vol.ensure(2 * vb));
    }
    if (need.vote) {
        SMX_HIP(c->varms.ensure(c->n * sizeof(uint32_t)));
        SMX_HIP(c->voted.ensure(fb));
        SMX_HIP(c->vote_ws.ensure(vote_workspace_bytes(c->w, c->h)));
    }
    if (need.adjust) SMX_HIP(c->adj_ws.ensure(adjust_workspace_bytes(c->w, c->h)));
    if (need.perm && !c->s.tree) SMX_HIP(c->perm_ws.ensure(ctx_perm_ws_bytes(c)));
    if (need.perm && c->s.tree) {
        SMX_HIP(c->tree_ws.ensure(ctx_tree_ws_bytes(c)));
        SMX_HIP(c->tree_dev.ensure(2 * smx_tree_bytes(c->w, c->h)));
    }
    if (need.bp) SMX_HIP(c->bp_ws.ensure(bp_workspace_bytes(c->w, c->h, c->size_d, c->s.bp_params.levels, 2)));
    if (need.pm) {
        SMX_HIP(c->pm_planes.ensure(6 * fb));
        SMX_HIP(c->pm_disp.ensure(2 * fb));
        SMX_HIP(c->pm_ws.ensure(pm_workspace_bytes(c->w, c->h)));
        SMX_HIP(c->subf.ensure(fb));
    }
    // The chunk of ctx_aggregate_chunks.  Colour guide and cross: the halving rule on their workspace.  The guided flow from
    // census codes: every slice with whole volumes, else what fits 1 GiB of cost slices exactly (at least one).  Then the
    // calling thread's smx_set_max_slices_per_launch bounds it, like the chunks inside every entry.
    size_t (*const mode_bytes)(int, int, int, int) = need.cgf ? cgf_workspace_bytes : need.cross ? cross_workspace_bytes : nullptr;
    c->chunk = c->size_d;
    if (mode_bytes) c->chunk = halved_chunk(c, mode_bytes, need.cost);
    else if (need.census && !need.cost) {
        const size_t fit = ((size_t)1 << 30) / (2 * fb);
        c->chunk = (int)(fit < 1 ? 1 : fit > (size_t)c->size_d ? (size_t)c->size_d : fit);
    }
    if (const int bound = thread_max_chunk(); bound > 0 && bound < c->chunk) c->chunk = bound;
    c->mode_ws_bytes = need.sgm ? sgm_workspace_bytes(c->w, c->h, c->size_d, 2) : mode_bytes ? mode_bytes(c->w, c->h, c->chunk, 2) : 0;
    if (c->mode_ws_bytes) SMX_HIP(c->mode_ws.ensure(c->mode_ws_bytes));
    if ((mode_bytes || need.census) && !need.cost) SMX_HIP(c->chunk_cost.ensure(2 * (size_t)c->chunk * fb));
    return SMX_OK;
}

// The census codes of both images of `call`: one launch where they lie back to back, else one per image.  With the ZNCC cost
// the window moments, in the same buffer and the same way.
static int ctx_census_codes(smx_ctx* c, const AggCall& call) {
    uint64_t* codes = c->codes.as<uint64_t>();
    if (c->s.cost_mode == SMX_COST_ZNCC) {
        if (call.guide[1] == call.guide[0] + c->n) return smx_dev_zncc_moments(&c->s.zncc, call.guide[0], codes, c->w, c->h, 2, call.st);
        int rc = SMX_OK;
        for (int v = 0; v < 2 && !rc; ++v) rc = smx_dev_zncc_moments(&c->s.zncc, call.guide[v], codes + v * c->n, c->w, c->h, 1, call.st);
        return rc;
    }
    const smx_census_params* cp = c->s.adcensus ? &c->s.adc.census : &c->s.census;
    if (call.guide[1] == call.guide[0] + c->n) return smx_dev_census(cp, call.guide[0], codes, c->w, c->h, 2, call.st);
    int rc = SMX_OK;
    for (int v = 0; v < 2 && !rc; ++v) rc = smx_dev_census(cp, call.guide[v], codes + v * c->n, c->w, c->h, 1, call.st);
    return rc;
}

// Slices [s0, s1) of both views' cost from the codes: the census cost, or AD-Census with its AD term from the gray images or
// from the colour images of the pair; or, without codes, the mutual-information cost from the table of the pass in hand; or
// the ZNCC cost from the moments and the gray images
static int ctx_code_cost(smx_ctx* c, const PairIn& in, float* cl, float* cr, int s0, int s1, hipStream_t st) {
    if (c->s.cost_mode == SMX_COST_ZNCC)
        return smx_dev_zncc_cost_pair(&c->s.zncc, c->codes.as<uint64_t>(), in.left, in.right, cl, cr, c->w, c->h, in.dminl, in.dminr, s0, s1, st);
    if (c->s.cost_mode == SMX_COST_MI)
        return smx_dev_mi_cost_pair(c->mi_table, in.left, in.right, cl, cr, c->w, c->h, in.dminl, in.dminr, s0, s1, st);
    const uint64_t* codes = c->codes.as<uint64_t>();
    if (!c->s.adcensus) return smx_dev_census_cost_pair(&c->s.census, codes, cl, cr, c->w, c->h, in.dminl, in.dminr, s0, s1, st);
    const bool colour = c->s.adc.colour != 0;
    return smx_dev_adcensus_cost_pair(&c->s.adc, c->adc_tab.as<float>(), codes, colour ? in.rgb_l : in.left,
                                      colour ? in.rgb_r : in.right, colour ? in.channels : 1, cl, cr, c->w, c->h, in.dminl,
                                      in.dminr, s0, s1, st);
}

// The opt-in aggregations of ctx_enqueue that go chunk by chunk -- the guided filter from census codes, the colour-guided
// filter, cross-based aggregation -- over ascending contiguous chunks [s0, s1) of the slices.  Per chunk: its cost slices of
// both views (from the codes, or the reference's; nothing where the whole reference volumes were built up front) into the
// whole volumes where the context holds them, else into the chunk buffer; then its aggregation, which accumulates into the
// keys and the states of `call`.
static int ctx_aggregate_chunks(smx_ctx* c, const PairIn& in, const AggCall& call, const PairPlan& need) {
    const size_t n = c->n;
    const int w = c->w, h = c->h, chunk = c->chunk;
    // cross-based: the guide is the colour pair where the pair came as colour images, else the gray pair
    const bool gray = need.cross && !in.channels;
    const uint8_t* gl = gray ? in.left : in.rgb_l;
    const uint8_t* gr = gray ? in.right : in.rgb_r;
    const int ch = gray ? 1 : in.channels;
    int rc;
    for (int s0 = 0; s0 < c->size_d; s0 += chunk) {
        const int s1 = s0 + chunk < c->size_d ? s0 + chunk : c->size_d;
        float* cl = need.cost ? c->costL.as<float>() + (size_t)s0 * n : c->chunk_cost.as<float>();
        float* cr = need.cost ? c->costR.as<float>() + (size_t)s0 * n : cl + (size_t)chunk * n;
        if (need.census) {
            if ((rc = ctx_code_cost(c, in, cl, cr, s0, s1, call.st))) return rc;
        } else if (!need.cost) {
            if ((rc = smx_dev_cost_volume(&c->p, in.left, in.right, cl, w, w, h, in.dminl, s0, s1, call.st))) return rc;
            if ((rc = smx_dev_cost_volume(&c->p, in.right, in.left, cr, w, w, h, in.dminr, s0, s1, call.st))) return rc;
        }
        float* agg[2] = {call.agg[0] ? call.agg[0] + (size_t)s0 * n : nullptr, call.agg[1] ? call.agg[1] + (size_t)s0 * n : nullptr};
        if (!need.cgf && !need.cross) {
            AggCall part = call;
            part.s_begin = s0; part.s_end = s1;
            part.cost[0] = cl; part.cost[1] = cr;
            part.agg[0] = agg[0]; part.agg[1] = agg[1];
            rc = run_aggregation(part, c->agg_path, s0 != 0);
        } else {
            // views l / r of the chunk into the outputs of view v; mode_ws_bytes, not the buffer's size: see smx_ctx
            auto views = [&](const uint8_t* l, const uint8_t* r, const float* kl, const float* kr, int v) {
                return need.cgf ? smx_dev_cgf_wta_pair(&c->p, l, r, ch, kl, kr, w, h, s0, s1, call.keys[v], agg[v], call.nbr[v],
                                                       call.uq[v], c->mode_ws.p, c->mode_ws_bytes, call.st)
                                : smx_dev_cross_wta_pair(&c->s.cross_params, l, r, ch, kl, kr, w, h, s0, s1, call.keys[v], agg[v],
                                                         call.nbr[v], call.uq[v], c->mode_ws.p, c->mode_ws_bytes, call.st);
            };
            // with the aggregated volumes wanted, view by view: the pair form lays its two views a chunk apart, the context a volume
            if (!need.agg) rc = views(gl, gr, cl, cr, 0);
            else if (!(rc = views(gl, nullptr, cl, nullptr, 0))) rc = views(nullptr, gr, nullptr, cr, 1);
        }
        if (rc) return rc;
    }
    return SMX_OK;
}

// The stages between the LR check and the sub-pixel maps: uniqueness, speckle removal, region voting, each followed by a fill
// that starts over from its map.  *kept: the map whose validity test says which pixels the fill replaced.
static int ctx_outlier_stages(smx_ctx* c, const PairIn& in, const PairPlan& need, const PairPlanes& out, const int64_t* keysL,
                              const float* uqL, const float** kept_out) {
    const smx_params* p = &c->p;
    const int w = c->w, h = c->h, size_d = c->size_d;
    const size_t n = c->n;
    hipStream_t st = c->st;
    int rc;
    const float* kept = out.occ;
    if (need.uniq) {
        // the ambiguous winners of the LR-checked left map join the invalidated pixels; the fill starts over from that map
        // (unless speckle removal follows, which does it)
        float* um = c->uq_map.as<float>();
        if ((rc = smx_dev_uniqueness(c->s.uniq, keysL, uqL, out.occ, um, c->uq_margin.as<float>(), w, h, (float)in.dminl,
                                     (float)(in.dminl - 100), st)))
            return rc;
        if (!need.speckle && (rc = launch_fill_occlusion(um, out.fil, w, h, (float)in.dminl, st))) return rc;
        kept = um;
    }
    if (need.speckle) {
        // the small components of the LR-checked map join the invalidated pixels; the fill starts over from that map
        float* spk = c->spk.as<float>();
        if ((rc = smx_dev_speckle_filter(&c->s.spk_params, kept, spk, w, h, (float)in.dminl, (float)(in.dminl - 100),
                                         c->spk_ws.p, speckle_workspace_bytes(w, h), st)))
            return rc;
        if ((rc = launch_fill_occlusion(spk, out.fil, w, h, (float)in.dminl, st))) return rc;
        kept = spk;
    }
    if (need.vote) {
        // the outliers of that map take the vote of their cross regions on the left guide, then the 16-direction interpolation;
        // the fill starts over from the voted map, and `kept` stays the map whose validity test the later stages read
        const uint8_t* guide = in.channels ? in.rgb_l : in.left;
        const int ch = in.channels ? in.channels : 1;
        uint32_t* arms = c->varms.as<uint32_t>();
        float* voted = c->voted.as<float>();
        if ((rc = smx_dev_cross_arms(&c->s.vote_arms, guide, nullptr, ch, w, h, arms, st))) return rc;
        if ((rc = smx_dev_region_vote(&c->s.vote_params, arms, guide, ch, kept, out.map + n, voted, w, h, in.dminl, size_d, p->d_lr,
                                      c->vote_ws.p, vote_workspace_bytes(w, h), st)))
            return rc;
        if ((rc = launch_fill_occlusion(voted, out.fil, w, h, (float)in.dminl, st))) return rc;
    }
    *kept_out = kept;
    return SMX_OK;
}

// A PatchMatch pair: the search gives both views' labels (dmap) and plane costs (best) directly; the LR check and the fill of
// main.cu:140-155 run on the labels, the outlier stages behind them unchanged, and the sub-pixel filled map is the left disp
// where the pixel was kept, the filled label elsewhere (the rule of smx_dev_subpixel_pair).
static int ctx_enqueue_pm(smx_ctx* c, const PairIn& in, const PairPlan& need, const PairPlanes& out) {
    const int w = c->w, h = c->h;
    const size_t n = c->n;
    hipStream_t st = c->st;
    int rc;
    float* disp = c->pm_disp.as<float>();
    if ((rc = smx_dev_patchmatch_pair(&c->p, &c->s.pm_params, in.left, in.right, w, h, c->size_d, in.dminl, in.dminr,
                                      c->pm_planes.as<float>(), out.best, disp, out.map, c->pm_ws.p, pm_workspace_bytes(w, h), st)))
        return rc;
    SMX_HIP(hipMemcpyAsync(out.occ, out.map, n * sizeof(float), hipMemcpyDeviceToDevice, st));
    if ((rc = launch_detect_occlusion(&c->p, out.occ, out.map + n, in.dminl - 100, w, h, st))) return rc;
    if ((rc = launch_fill_occlusion(out.occ, out.fil, w, h, (float)in.dminl, st))) return rc;
    const float* kept = nullptr;
    if ((rc = ctx_outlier_stages(c, in, need, out, nullptr, nullptr, &kept))) return rc;
    return launch_pm_sub_filled(disp, kept, out.fil, n, in.dminl, c->subf.as<float>(), st);
}

// The path of one pair on the context's stream: device images in, the eight result planes (+ the context's volumes) out.
static int ctx_enqueue(smx_ctx* c, const PairIn& in, const PairPlan& need, const PairPlanes& out) {
    if (need.pm) return ctx_enqueue_pm(c, in, need, out);
    const smx_params* p = &c->p;
    const int w = c->w, h = c->h, size_d = c->size_d;
    const size_t n = c->n;
    hipStream_t st = c->st;
    int rc;
    int64_t* keysL = c->keys.as<int64_t>();
    // cost volumes are materialised only when the caller asks for them (main.cu:80-82) or SGM reads them, and then feed
    // the aggregation like in the reference; otherwise the slices are built on the fly inside it.
    float* const costL = need.cost ? c->costL.as<float>() : nullptr;
    float* const costR = need.cost ? c->costR.as<float>() : nullptr;
    float* const aggL = need.agg ? c->aggLR.as<float>() : nullptr;
    float* const nbrL = need.subpix ? c->nbr.as<float>() : nullptr;
    float* const uqL = need.uniq ? c->uq.as<float>() : nullptr;     // (no initialisation: the keys start as the identity)
    if (need.cost && !need.census) {
        if ((rc = smx_dev_cost_volume(p, in.left, in.right, costL, w, w, h, in.dminl, 0, size_d, st))) return rc;
        if ((rc = smx_dev_cost_volume(p, in.right, in.left, costR, w, w, h, in.dminr, 0, size_d, st))) return rc;
    }
    if ((rc = smx_dev_init_keys(keysL, 2 * (int64_t)n, st))) return rc;
    // (with cross-scale or the permeability filter the states come from that pass: the aggregation keeps none.  Its keys are
    // overwritten too, but the fused aggregation has no form without its winner-take-all pass.)
    float* const nbrA = need.cscale || need.perm ? nullptr : nbrL;
    float* const uqA = need.cscale || need.perm ? nullptr : uqL;
    // main.cu:133-134, both views per call, on the context's own path
    const AggCall call = {"smx_ctx_stereo_pair", p, 2, {in.left, in.right}, {in.right, in.left}, {costL, costR},
                          {in.dminl, in.dminr}, {keysL, keysL + n}, {out.mean, out.mean + n},
                          {aggL, need.agg ? aggL + (size_t)size_d * n : nullptr}, {nbrA, nbrA ? nbrA + 3 * n : nullptr},
                          {uqA, uqA ? uqA + 3 * n : nullptr}, w, h, 0, size_d, c->ws.p, c->ws_bytes, st};
    if (need.census && c->s.cost_mode != SMX_COST_MI && (rc = ctx_census_codes(c, call))) return rc;
    if (need.sgm) {
        // SGM instead of the guided filter: it reads the whole volumes, the census ones come from one launch
        if (need.census) rc = ctx_code_cost(c, in, costL, costR, 0, size_d, st);
        if (!rc) rc = need.uniq ? smx_dev_sgm_wta_pair_uq(&c->s.sgm, costL, costR, w, h, size_d, keysL, aggL, nbrL, uqL, c->mode_ws.p,
                                                          c->mode_ws_bytes, st)
                                : smx_dev_sgm_wta_pair(&c->s.sgm, costL, costR, w, h, size_d, keysL, aggL, nbrL, c->mode_ws.p,
                                                       c->mode_ws_bytes, st);
    } else if (need.bp) {
        // belief propagation instead of the guided filter: the flow of SGM, the uniqueness state from the same call
        if (need.census) rc = ctx_code_cost(c, in, costL, costR, 0, size_d, st);
        if (!rc) rc = smx_dev_bp_wta_pair(&c->s.bp_params, costL, costR, w, h, size_d, keysL, aggL, nbrL, uqL, c->bp_ws.p, c->bp_ws.bytes, st);
    } else if (need.so) {
        // the scan-line optimiser reads whole volumes: the cost volumes, as SGM does, or behind cross-based aggregation the
        // two volumes of its q, collected over the chunks with the keys of that pass discarded (the optimiser's are OUT only)
        const uint8_t* gl = in.channels ? in.rgb_l : in.left;
        const uint8_t* gr = in.channels ? in.rgb_r : in.right;
        const float* vl = costL;
        const float* vr = costR;
        if (need.cross) {
            float* vol = c->so_vol.as<float>();
            AggCall chain = call;
            PairPlan cn = need;
            cn.agg = true;
            chain.agg[0] = vol; chain.agg[1] = vol + (size_t)size_d * n;
            chain.nbr[0] = chain.nbr[1] = chain.uq[0] = chain.uq[1] = nullptr;
            rc = ctx_aggregate_chunks(c, in, chain, cn);
            vl = vol; vr = vol + (size_t)size_d * n;
        } else if (need.census) rc = ctx_code_cost(c, in, costL, costR, 0, size_d, st);
        if (!rc) rc = smx_dev_scanline_wta_pair(&c->s.so_params, gl, gr, in.channels ? in.channels : 1, vl, vr, w, h, size_d, in.dminl,
                                                in.dminr, keysL, aggL, nbrL, uqL, c->so_ws.p, c->so_ws.bytes, st);
    } else if (need.cgf || need.cross || need.census) rc = ctx_aggregate_chunks(c, in, call, need);
    else rc = run_aggregation(call, c->agg_path, false);
    if (rc) return rc;
    if (need.level) return SMX_OK;
    if (need.cscale) {
        // the levels' volumes are on the stream already (ctx_cscale_levels): the combination goes over the level-0 volumes,
        // and its winners and states take the place of the plain ones
        const float* al[SMX_CSCALE_MAX_SCALES] = {aggL};
        const float* ar[SMX_CSCALE_MAX_SCALES] = {aggL + (size_t)size_d * n};
        for (int s = 1; s < c->s.cs_params.scales; ++s) {
            smx_ctx* k = c->cs_child[s];
            al[s] = k->aggLR.as<float>();
            ar[s] = al[s] + (size_t)k->size_d * k->n;
        }
        if ((rc = smx_dev_cscale_wta_pair(&c->s.cs_params, al, ar, w, h, in.dminl, in.dminr, size_d, keysL, aggL, nbrL, uqL, st)))
            return rc;
    }
    if (need.perm && c->s.tree) {
        // the tree filter in the same place, over the two trees that ctx_pair built from the pair's guides and uploaded
        const uint8_t* trees = c->tree_dev.as<uint8_t>();
        if ((rc = smx_dev_tree_wta_pair(&c->s.tree_params, aggL, aggL + (size_t)size_d * n, trees, trees + smx_tree_bytes(w, h), w, h,
                                        in.dminl, in.dminr, size_d, keysL, aggL, nbrL, uqL, c->tree_ws.p, ctx_tree_ws_bytes(c), st)))
            return rc;
    } else if (need.perm) {
        // the filter goes over both aggregated volumes in place; its winners and states take the place of the plain ones
        const bool colour = need.cgf;
        if ((rc = smx_dev_permeability_wta_pair(&c->s.perm_params, aggL, aggL + (size_t)size_d * n, colour ? in.rgb_l : in.left,
                                                colour ? in.rgb_r : in.right, colour ? in.channels : 1, w, h, in.dminl, in.dminr,
                                                size_d, keysL, aggL, nbrL, uqL, c->perm_ws.p, ctx_perm_ws_bytes(c), st)))
            return rc;
    }
    // main.cu:112-118 presets, winning slices, main.cu:140-155
    if ((rc = smx_dev_finish_pair(p, keysL, w, h, in.dminl, in.dminr, in.dminl - 100, (float)in.dminl, out.best, out.map,
                                  out.occ, out.fil, st)))
        return rc;
    const float* kept = nullptr;
    if ((rc = ctx_outlier_stages(c, in, need, out, keysL, uqL, &kept))) return rc;
    if (need.subpix && (rc = smx_dev_subpixel_pair(c->s.subpix, keysL, nbrL, out.map, kept, out.fil, w, h, in.dminl,
                                                   c->sub.as<float>(), c->subf.as<float>(), st)))
        return rc;
    if (!need.adjust) return SMX_OK;
    // the filled map looks at the left volume again: a pixel beside a depth step takes the neighbour's label where that costs
    // it less, in place, and its entry of the sub-pixel filled map becomes its own fit; `kept` is not replaced
    return smx_dev_discontinuity_adjust(&c->s.adj_params, out.fil, aggL, out.fil, w, h, in.dminl, size_d, c->s.subpix,
                                        need.subpix ? c->subf.as<float>() : nullptr, c->adj_ws.p, adjust_workspace_bytes(w, h), st);
}

static int ctx_create(const smx_params* p, int w, int h, int size_d, hipStream_t shared, smx_ctx** out);
static int ctx_adcensus_table(smx_ctx* c);

// Levels 1 .. scales-1 of a cross-scale pair: each level's images from the level below (the gray pyramid from the gray images,
// the colour pyramid from the colour images), then the level's pair through ctx_enqueue on a child context that takes this
// context's settings.  Both views of a level run with the larger of the two views' slice counts; the slices past a view's own
// range are not read by the combination.
static int ctx_cscale_levels(smx_ctx* c, const char* who, const PairIn& in, const PairPlan& need) {
    int rc;
    const smx_ctx* below = c;
    PairIn src = in;
    for (int s = 1; s < c->s.cs_params.scales; ++s) {
        int ws, hs, dl, dr, sl, sr;
        cscale_level(c->w, c->h, in.dminl, c->size_d, s, &ws, &hs, &dl, &sl);
        cscale_level(c->w, c->h, in.dminr, c->size_d, s, &ws, &hs, &dr, &sr);
        const int sd = sl > sr ? sl : sr;
        if (ws < 2) return fail(SMX_E_ARG, "%s: cross-scale level %d of a %d x %d pair is narrower than 2 pixels", who, s, c->w, c->h);
        smx_ctx*& k = c->cs_child[s];
        if (k && k->size_d != sd) { delete k; k = nullptr; }
        if (!k && (rc = ctx_create(&c->p, ws, hs, sd, c->st, &k))) return rc;
        k->p = c->p;
        k->agg_path = c->agg_path;
        k->s.cost_mode = c->s.cost_mode;
        k->s.census = c->s.census;
        k->s.zncc = c->s.zncc;
        k->s.guide_mode = c->s.guide_mode;
        if (c->s.adcensus && (!k->s.adcensus || memcmp(&k->s.adc, &c->s.adc, sizeof(k->s.adc)) != 0)) { k->s.adc = c->s.adc; k->adc_tab_valid = false; }
        k->s.adcensus = c->s.adcensus;
        k->mi_table = c->mi_table;
        PairPlan kn = {};
        kn.agg = kn.level = true;
        kn.census = need.census;
        kn.cgf = need.cgf;
        if (kn.cgf && !stage_shape_ok(STAGES[S_CGF], ws, hs, 1, 0, 0))
            return fail(SMX_E_ARG, "%s: the colour-guided filter does not take cross-scale level %d", who, s);
        if ((rc = ctx_reserve(k, kn))) return rc;
        if ((rc = ctx_adcensus_table(k))) return rc;
        uint8_t* gl = k->dL.as<uint8_t>(); uint8_t* gr = k->dR.as<uint8_t>();
        if ((rc = smx_dev_pyr_down(src.left, gl, below->w, below->h, 1, c->st))) return rc;
        if ((rc = smx_dev_pyr_down(src.right, gr, below->w, below->h, 1, c->st))) return rc;
        uint8_t *cl = nullptr, *cr = nullptr;
        if (in.channels) {
            SMX_HIP(k->rgb.ensure(2 * k->n * (size_t)in.channels));
            cl = k->rgb.as<uint8_t>(); cr = cl + k->n * (size_t)in.channels;
            if ((rc = smx_dev_pyr_down(src.rgb_l, cl, below->w, below->h, in.channels, c->st))) return rc;
            if ((rc = smx_dev_pyr_down(src.rgb_r, cr, below->w, below->h, in.channels, c->st))) return rc;
        }
        src = {gl, gr, dl, dr, cl, cr, in.channels};
        if ((rc = ctx_enqueue(k, src, kn, {k->best.as<float>(), k->map.as<float>(), k->mean.as<uint8_t>(), k->occ.as<float>(),
                                           k->fil.as<float>()})))
            return rc;
        below = k;
    }
    return SMX_OK;
}

static int ctx_check_device(smx_ctx* c, const char* who) {
    int dev = -1;
    SMX_HIP(hipGetDevice(&dev));
    if (dev != c->dev) return fail(SMX_E_ARG, "%s: the context lives on device %d, current device is %d", who, c->dev, dev);
    return SMX_OK;
}

// The planes of a smx_pair_out in the order of the struct -- the eight result planes, then the four volumes -- with their bytes
// per pixel.  Both entries copy `from` one such struct `to` another through this table; a NULL plane is skipped.
struct PlaneRef { void* p; size_t elem; };
static std::array<PlaneRef, 12> pair_planes(const smx_pair_out& o, size_t size_d) {
    const size_t f = sizeof(float), v = f * size_d;
    return {{{o.best_l, f}, {o.best_r, f}, {o.dmap_l, f}, {o.dmap_r, f}, {o.mean_l, 1}, {o.mean_r, 1}, {o.occlusion, f},
             {o.filled, f}, {o.cost_l, v}, {o.cost_r, v}, {o.agg_l, v}, {o.agg_r, v}}};
}

// shared: NULL, or the stream of the parent context of this pyramid level
static int ctx_create(const smx_params* p, int w, int h, int size_d, hipStream_t shared, smx_ctx** out) {
    *out = nullptr;
    smx_ctx* c = new (std::nothrow) smx_ctx;
    if (!c) return fail(SMX_E_HIP, "smx_create: out of host memory");
    struct Guard { smx_ctx* c; ~Guard() { delete c; } } guard{c};
    c->p = *p; c->w = w; c->h = h; c->size_d = size_d;
    c->agg_path = thread_agg_path();
    c->n = (size_t)w * h;
    const size_t n = c->n, fb = n * sizeof(float);
    SMX_HIP(hipGetDevice(&c->dev));
    if (shared) { c->st = shared; c->owns_st = false; }
    else SMX_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c->ws_bytes = 2 * pick_ws_bytes(w, h, size_d);     // both views per launch
    SMX_HIP(c->dL.ensure(n)); SMX_HIP(c->dR.ensure(n));
    SMX_HIP(c->keys.ensure(2 * n * 8));
    SMX_HIP(c->best.ensure(2 * fb)); SMX_HIP(c->map.ensure(2 * fb));
    SMX_HIP(c->mean.ensure(2 * n));
    SMX_HIP(c->occ.ensure(fb)); SMX_HIP(c->fil.ensure(fb));
    SMX_HIP(c->ws.ensure(c->ws_bytes));
    guard.c = nullptr;
    *out = c;
    return SMX_OK;
}

// The device table of the AD-Census cost, built where the context's parameters changed
static int ctx_adcensus_table(smx_ctx* c) {
    if (!c->s.adcensus || c->adc_tab_valid) return SMX_OK;
    SMX_HIP(c->adc_tab.ensure(SMX_ADCENSUS_TABLE_FLOATS * sizeof(float)));
    if (int rc = smx_dev_adcensus_tables(&c->s.adc, c->adc_tab.as<float>(), c->st)) return rc;
    c->adc_tab_valid = true;
    return SMX_OK;
}

extern "C" {

int smx_create(const smx_params* p, int w, int h, int size_d, smx_ctx** out) {
    SMX_ARG(p && out && w >= 2 && h >= 1 && size_d >= 1 && p->radius >= 0);
    return ctx_create(p, w, h, size_d, nullptr, out);
}

int smx_ctx_set_agg_path(smx_ctx* c, int path) {
    SMX_ARG(c);
    if (path < 0 || path > 5) return fail(SMX_E_ARG, "smx_ctx_set_agg_path: path must be 0 .. 5");
    c->agg_path = path;
    return SMX_OK;
}

int smx_destroy(smx_ctx* c) {
    if (!c) return SMX_OK;
    int dev = -1;
    (void)hipGetDevice(&dev);
    if (c->dev >= 0 && dev != c->dev) (void)hipSetDevice(c->dev);
    for (hipStream_t x : {c->st_up, c->st, c->st_dn})
        if (x) (void)hipStreamSynchronize(x);
    delete c;
    if (dev >= 0) (void)hipSetDevice(dev);
    return SMX_OK;
}

}  // extern "C"

// The synchronous pair entry on gray images (channels == 0: img_l / img_r are the gray images) or on colour images, whose
// gray images for the cost are made on the device.
static int ctx_pair(smx_ctx* c, const uint8_t* img_l, const uint8_t* img_r, int channels, int dminl, int dminr, const smx_pair_out* out) {
    const PairEntry entry = channels ? ENTRY_RGB : ENTRY_GRAY;
    const char* who = ENTRY_NAMES[entry];
    const size_t n = c->n;
    int rc;
    if ((rc = ctx_check_device(c, who))) return rc;
    if (c->submitted != c->waited) return fail(SMX_E_ARG, "%s: pipelined pairs are still in flight (smx_ctx_wait)", who);
    hipStream_t st = c->st;
    PairPlan need;
    char why[512];
    if (plan_pair(c->s, c->w, c->h, c->size_d, entry, channels, dminl, dminr, out->cost_l || out->cost_r,
                  out->agg_l || out->agg_r, out->mean_l || out->mean_r, &need, why, sizeof(why)))
        return fail(SMX_E_ARG, "%s", why);
    if ((rc = ctx_reserve(c, need))) return rc;
    if ((rc = ctx_adcensus_table(c))) return rc;
    if (channels) SMX_HIP(c->rgb.ensure(2 * n * (size_t)channels));
    c->done = PairPlan{};
    c->done_mi = false;
    uint8_t* dL = c->dL.as<uint8_t>(); uint8_t* dR = c->dR.as<uint8_t>();
    uint8_t* rgbL = channels ? c->rgb.as<uint8_t>() : nullptr;
    uint8_t* rgbR = channels ? rgbL + n * (size_t)channels : nullptr;
    stage_mark(ST_BEGIN, st);
    if (channels) {
        SMX_HIP(hipMemcpyAsync(rgbL, img_l, n * (size_t)channels, hipMemcpyHostToDevice, st));
        SMX_HIP(hipMemcpyAsync(rgbR, img_r, n * (size_t)channels, hipMemcpyHostToDevice, st));
        if ((rc = smx_dev_rgb_to_grayscale(&c->p, rgbL, (int64_t)n, channels, dL, st))) return rc;
        if ((rc = smx_dev_rgb_to_grayscale(&c->p, rgbR, (int64_t)n, channels, dR, st))) return rc;
    } else {
        SMX_HIP(hipMemcpyAsync(dL, img_l, n, hipMemcpyHostToDevice, st));
        SMX_HIP(hipMemcpyAsync(dR, img_r, n, hipMemcpyHostToDevice, st));
    }
    if (need.perm && c->s.tree) {
        // the two trees, on the host from the pair's guides -- the images as they came, or the device's gray images of a colour
        // pair under the gray guide, fetched for it -- then up behind the images
        const size_t tb = smx_tree_bytes(c->w, c->h);
        const uint8_t* gl = img_l;
        const uint8_t* gr = img_r;
        int gch = channels ? channels : 1;
        try {
            c->tree_host.resize(2 * (tb / 4));
            if (channels && !need.cgf) c->tree_gray.resize(2 * n);
        } catch (const std::bad_alloc&) {
            return fail(SMX_E_HIP, "%s: out of host memory for the trees", who);
        }
        if (channels && !need.cgf) {
            SMX_HIP(hipMemcpyAsync(c->tree_gray.data(), dL, n, hipMemcpyDeviceToHost, st));
            SMX_HIP(hipMemcpyAsync(c->tree_gray.data() + n, dR, n, hipMemcpyDeviceToHost, st));
            SMX_HIP(hipStreamSynchronize(st));
            gl = c->tree_gray.data(); gr = gl + n; gch = 1;
        }
        uint32_t* blobs = c->tree_host.data();
        if ((rc = smx_tree_build(gl, gch, c->w, c->h, blobs))) return rc;
        if ((rc = smx_tree_build(gr, gch, c->w, c->h, blobs + tb / 4))) return rc;
        SMX_HIP(hipMemcpyAsync(c->tree_dev.p, blobs, 2 * tb, hipMemcpyHostToDevice, st));
    }
    stage_mark(ST_UPLOAD, st);
    float* best = c->best.as<float>(); float* map = c->map.as<float>(); float* agg = c->aggLR.as<float>();
    uint8_t* mean = c->mean.as<uint8_t>();
    const PairIn in = {dL, dR, dminl, dminr, rgbL, rgbR, channels};
    const PairPlanes planes = {best, map, mean, c->occ.as<float>(), c->fil.as<float>()};
    // one pass of the pair under a plan (the chunk and the workspace's share are per plan: ctx_reserve)
    auto pass = [&](const PairPlan& pl) {
        int r = ctx_reserve(c, pl);
        if (!r && pl.cscale) r = ctx_cscale_levels(c, who, in, pl);
        return r ? r : ctx_enqueue(c, in, pl, planes);
    };
    if (c->s.cost_mode == SMX_COST_MI) {
        // include/smx.h, smx_ctx_set_mi: the start map, then per table a histogram of the current LR-checked left map, its
        // table by way of the host, and -- before the last table -- a pass that stops behind the LR check and the fill
        const smx_mi_params& mp = c->s.mi;
        const size_t cells = (size_t)SMX_MI_LEVELS * SMX_MI_LEVELS;
        PairPlan early = need;
        early.uniq = early.speckle = early.vote = early.subpix = early.adjust = false;
        if (mp.init == SMX_MI_INIT_REFERENCE) {
            PairPlan start = early;
            start.census = false;                       // (no cost from a table: the reference's, in the same flow)
            rc = pass(start);
        } else rc = smx_dev_mi_random_map(planes.occ, c->w, c->h, dminl, c->size_d, mp.seed, st);
        if (rc) return rc;
        std::vector<uint32_t> hist(cells);
        for (int k = 1; k <= mp.iterations; ++k) {
            if ((rc = smx_dev_mi_histogram(dL, dR, planes.occ, (float)(dminl - 100), c->mi_hist.as<uint32_t>(), c->w, c->h, st))) return rc;
            SMX_HIP(hipMemcpyAsync(hist.data(), c->mi_hist.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            SMX_HIP(hipStreamSynchronize(st));
            if ((rc = smx_dev_mi_table(hist.data(), c->mi_tab.as<uint8_t>(), st))) return rc;
            if (k < mp.iterations && (rc = pass(early))) return rc;
        }
    }
    if ((rc = pass(need))) return rc;
    const smx_pair_out dev = {best, best + n, map, map + n, mean, mean + n, c->occ.as<float>(), c->fil.as<float>(),
                              c->costL.as<float>(), c->costR.as<float>(), agg, need.agg ? agg + c->size_d * n : nullptr};
    const auto to = pair_planes(*out, c->size_d), from = pair_planes(dev, c->size_d);
    for (size_t i = 0; i < to.size(); ++i)
        if (to[i].p && from[i].p) SMX_HIP(hipMemcpyAsync(to[i].p, from[i].p, n * from[i].elem, hipMemcpyDeviceToHost, st));
    stage_mark(ST_DOWNLOAD, st);
    SMX_HIP(hipStreamSynchronize(st));
    // (only the fused aggregation waits for a hand-over, and reports one that timed out)
    if (need.walker_status) {
        if ((rc = smx_dev_agg_status(c->ws.p))) return rc;
        for (int s = 1; need.cscale && s < c->s.cs_params.scales; ++s)
            if ((rc = smx_dev_agg_status(c->cs_child[s]->ws.p))) return rc;
    }
    c->done = need;
    c->done_mi = c->s.cost_mode == SMX_COST_MI;
    return SMX_OK;
}

extern "C" {

int smx_ctx_stereo_pair(smx_ctx* c, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr,
                        const smx_pair_out* out) {
    SMX_ARG(c && gray_l && gray_r && out);
    return ctx_pair(c, gray_l, gray_r, 0, dminl, dminr, out);
}

int smx_ctx_stereo_pair_rgb(smx_ctx* c, const uint8_t* rgb_l, const uint8_t* rgb_r, int channels, int dminl, int dminr,
                            const smx_pair_out* out) {
    SMX_ARG(c && rgb_l && rgb_r && out && (channels == 3 || channels == 4));
    return ctx_pair(c, rgb_l, rgb_r, channels, dminl, dminr, out);
}

// ---- the setters.  Those that switch a stage on with a params struct and off with NULL share ctx_set_stage: the struct is
// validated and copied, the stage's shape limit checked where its row says AT_SETTER, and a refused call changes nothing.
}  // extern "C"

template <class P>
static int ctx_set_stage(smx_ctx* c, CtxStage id, bool CtxSettings::*on, P CtxSettings::*slot, const P* p, bool (*params_ok)(const P*),
                         const char* ranges) {
    SMX_ARG(c);
    const StageRow& row = STAGES[id];
    if (p) {
        if (!params_ok(p)) return fail(SMX_E_ARG, "%s: %s", row.setter, ranges);
        if ((row.limit.checked & AT_SETTER) && !stage_shape_ok(row, c->w, c->h, c->size_d, 0, 0))
            return fail(SMX_E_ARG, "%s: %s", row.setter, row.limit.shapes);
        c->s.*slot = *p;
    }
    c->s.*on = p != nullptr;
    return SMX_OK;
}

extern "C" {

// (the permeability filter and the tree filter are the two modes of one row: a setter refuses to switch its mode on over the other)
int smx_ctx_set_permeability(smx_ctx* c, const smx_perm_params* p) {
    SMX_ARG(c);
    if (const char* why = p ? row_mode_conflict(c->s, false) : nullptr) return fail(SMX_E_ARG, "%s", why);
    return ctx_set_stage(c, S_PERM, &CtxSettings::perm, &CtxSettings::perm_params, p, perm_params_ok, PERM_RANGES);
}
int smx_ctx_set_tree(smx_ctx* c, const smx_tree_params* p) {
    SMX_ARG(c);
    if (p && !tree_params_ok(p)) return fail(SMX_E_ARG, "smx_ctx_set_tree: %s", TREE_RANGES);
    if (const char* why = p ? row_mode_conflict(c->s, true) : nullptr) return fail(SMX_E_ARG, "%s", why);
    return ctx_set_stage(c, S_PERM, &CtxSettings::tree, &CtxSettings::tree_params, p, tree_params_ok, TREE_RANGES);
}
int smx_ctx_set_bp(smx_ctx* c, const smx_bp_params* p) {
    return ctx_set_stage(c, S_BP, &CtxSettings::bp, &CtxSettings::bp_params, p, bp_params_ok, BP_RANGES);
}
int smx_ctx_set_cross(smx_ctx* c, const smx_cross_params* p) {
    return ctx_set_stage(c, S_CROSS, &CtxSettings::cross, &CtxSettings::cross_params, p, cross_params_ok, CROSS_RANGES);
}
int smx_ctx_set_scanline(smx_ctx* c, const smx_scanline_params* p) {
    return ctx_set_stage(c, S_SO, &CtxSettings::so, &CtxSettings::so_params, p, scanline_params_ok, SCANLINE_RANGES);
}
int smx_ctx_set_speckle(smx_ctx* c, const smx_speckle_params* p) {
    return ctx_set_stage(c, S_SPECKLE, &CtxSettings::speckle, &CtxSettings::spk_params, p, speckle_params_ok, SPECKLE_RANGES);
}
int smx_ctx_set_adjust(smx_ctx* c, const smx_adjust_params* p) {
    return ctx_set_stage(c, S_ADJUST, &CtxSettings::adjust, &CtxSettings::adj_params, p, adjust_params_ok, ADJUST_RANGES);
}
int smx_ctx_set_cross_scale(smx_ctx* c, const smx_cscale_params* p) {
    return ctx_set_stage(c, S_CSCALE, &CtxSettings::cscale, &CtxSettings::cs_params, p, cscale_params_ok, CSCALE_RANGES);
}
int smx_ctx_set_patchmatch(smx_ctx* c, const smx_pm_params* p) {
    return ctx_set_stage(c, S_PM, &CtxSettings::pm, &CtxSettings::pm_params, p, pm_params_ok, PM_RANGES);
}

int smx_ctx_set_vote(smx_ctx* c, const smx_vote_params* vote, const smx_cross_params* cross) {
    SMX_ARG(c);
    if (vote) {
        if (!vote_params_ok(vote)) return fail(SMX_E_ARG, "smx_ctx_set_vote: %s", VOTE_RANGES);
        smx_cross_params cp;
        smx_default_cross_params(&cp);
        if (cross) { cp = *cross; cp.iterations = 1; }
        if (!cross_params_ok(&cp)) return fail(SMX_E_ARG, "smx_ctx_set_vote: the arms: %s", CROSS_RANGES);
        if (!stage_shape_ok(STAGES[S_VOTE], c->w, c->h, c->size_d, 0, 0)) return fail(SMX_E_ARG, "smx_ctx_set_vote: %s", VOTE_SHAPES);
        c->s.vote_params = *vote;
        c->s.vote_arms = cp;
    }
    c->s.vote = vote != nullptr;
    return SMX_OK;
}

int smx_ctx_set_guidance(smx_ctx* c, int mode) {
    SMX_ARG(c);
    if (mode != SMX_GUIDE_GRAY && mode != SMX_GUIDE_RGB)
        return fail(SMX_E_ARG, "smx_ctx_set_guidance: mode must be SMX_GUIDE_GRAY or SMX_GUIDE_RGB");
    c->s.guide_mode = mode;
    return SMX_OK;
}

int smx_ctx_set_subpixel(smx_ctx* c, int mode) {
    SMX_ARG(c);
    if (mode != 0 && !subpix_mode_ok(mode))
        return fail(SMX_E_ARG, "smx_ctx_set_subpixel: mode must be 0, SMX_SUBPIX_PARABOLA or SMX_SUBPIX_EQUIANGULAR");
    c->s.subpix = mode;
    return SMX_OK;
}

int smx_ctx_set_uniqueness(smx_ctx* c, float ratio) {
    SMX_ARG(c);
    if (!uniq_ratio_ok(ratio)) return fail(SMX_E_ARG, "smx_ctx_set_uniqueness: the ratio must be finite and >= 0 (0 = off)");
    c->s.uniq = ratio;
    return SMX_OK;
}

int smx_ctx_set_cost(smx_ctx* c, int mode, const smx_census_params* census) {
    SMX_ARG(c);
    if (mode != SMX_COST_REFERENCE && mode != SMX_COST_CENSUS)
        return fail(SMX_E_ARG, "smx_ctx_set_cost: mode must be SMX_COST_REFERENCE or SMX_COST_CENSUS");
    if (mode == SMX_COST_CENSUS) {
        smx_census_params p;
        smx_default_census_params(&p);
        if (census) p = *census;
        if (!census_params_ok(&p)) return fail(SMX_E_ARG, "smx_ctx_set_cost: %s", CENSUS_RANGES);
        c->s.census = p;
    }
    c->s.cost_mode = mode;
    c->s.adcensus = false;
    return SMX_OK;
}

int smx_ctx_set_adcensus(smx_ctx* c, const smx_adcensus_params* p) {
    SMX_ARG(c);
    if (p) {
        if (!adcensus_params_ok(p)) return fail(SMX_E_ARG, "smx_ctx_set_adcensus: %s", ADCENSUS_RANGES);
        c->s.adc = *p;
        c->adc_tab_valid = false;
        c->s.cost_mode = SMX_COST_REFERENCE;      // (it replaces whatever smx_ctx_set_cost chose)
    }
    c->s.adcensus = p != nullptr;
    return SMX_OK;
}

int smx_ctx_set_mi(smx_ctx* c, const smx_mi_params* p) {
    SMX_ARG(c);
    if (p) {
        if (p->iterations < 1 || p->iterations > 16 || (p->init != SMX_MI_INIT_RANDOM && p->init != SMX_MI_INIT_REFERENCE))
            return fail(SMX_E_ARG, "smx_ctx_set_mi: needs 1 <= iterations <= 16 and init SMX_MI_INIT_RANDOM or SMX_MI_INIT_REFERENCE");
        c->s.mi = *p;
        c->s.cost_mode = SMX_COST_MI;                   // (it replaces whatever smx_ctx_set_cost or smx_ctx_set_adcensus chose)
        c->s.adcensus = false;
    } else if (c->s.cost_mode == SMX_COST_MI) c->s.cost_mode = SMX_COST_REFERENCE;
    return SMX_OK;
}

int smx_ctx_set_zncc(smx_ctx* c, const smx_zncc_params* p) {
    SMX_ARG(c);
    if (p) {
        if (!zncc_params_ok(p)) return fail(SMX_E_ARG, "smx_ctx_set_zncc: %s", ZNCC_RANGES);
        c->s.zncc = *p;
        c->s.cost_mode = SMX_COST_ZNCC;                 // (it replaces whatever the other cost setters chose)
        c->s.adcensus = false;
    } else if (c->s.cost_mode == SMX_COST_ZNCC) c->s.cost_mode = SMX_COST_REFERENCE;
    return SMX_OK;
}

int smx_ctx_set_aggregation(smx_ctx* c, int mode, const smx_sgm_params* sgm) {
    SMX_ARG(c);
    if (mode != SMX_AGG_GUIDED && mode != SMX_AGG_SGM)
        return fail(SMX_E_ARG, "smx_ctx_set_aggregation: mode must be SMX_AGG_GUIDED or SMX_AGG_SGM");
    if (mode == SMX_AGG_SGM) {
        smx_sgm_params p;
        smx_default_sgm_params(&p);
        if (sgm) p = *sgm;
        if (!sgm_params_ok(&p)) return fail(SMX_E_ARG, "smx_ctx_set_aggregation: SGM %s", SGM_RANGES);
        if (!stage_shape_ok(STAGES[S_SGM], c->w, c->h, c->size_d, 0, 0)) return fail(SMX_E_ARG, "smx_ctx_set_aggregation: SGM %s", SGM_SHAPES);
        c->s.sgm = p;
    }
    c->s.agg_mode = mode;
    return SMX_OK;
}

// ---- the maps of the last synchronous pair (c->done says which stages it ran) --------------------------------------------------
int smx_ctx_speckle_map(smx_ctx* c, float* despeckled) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_speckle_map")) return rc;
    if (!c->done.speckle) return fail(SMX_E_ARG, "smx_ctx_speckle_map: the last smx_ctx_stereo_pair ran without speckle removal");
    if (despeckled) SMX_HIP(c->spk.download(despeckled, c->n * sizeof(float)));
    return SMX_OK;
}

int smx_ctx_vote_map(smx_ctx* c, float* voted) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_vote_map")) return rc;
    if (!c->done.vote) return fail(SMX_E_ARG, "smx_ctx_vote_map: the last smx_ctx_stereo_pair ran without region voting");
    if (voted) SMX_HIP(c->voted.download(voted, c->n * sizeof(float)));
    return SMX_OK;
}

int smx_ctx_uniqueness_map(smx_ctx* c, float* map, float* margin) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_uniqueness_map")) return rc;
    if (!c->done.uniq) return fail(SMX_E_ARG, "smx_ctx_uniqueness_map: the last smx_ctx_stereo_pair ran without the uniqueness test");
    if (map) SMX_HIP(c->uq_map.download(map, c->n * sizeof(float)));
    if (margin) SMX_HIP(c->uq_margin.download(margin, c->n * sizeof(float)));
    return SMX_OK;
}

int smx_ctx_mi_table(smx_ctx* c, uint8_t* table, uint32_t* hist) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_mi_table")) return rc;
    if (!c->done_mi) return fail(SMX_E_ARG, "smx_ctx_mi_table: the last smx_ctx_stereo_pair ran without the mutual-information cost");
    const size_t cells = (size_t)SMX_MI_LEVELS * SMX_MI_LEVELS;
    if (table) SMX_HIP(c->mi_tab.download(table, cells));
    if (hist) SMX_HIP(c->mi_hist.download(hist, cells * sizeof(uint32_t)));
    return SMX_OK;
}

int smx_ctx_subpixel_maps(smx_ctx* c, float* sub_l, float* sub_r, float* sub_filled) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_subpixel_maps")) return rc;
    if (!c->done.subpix) return fail(SMX_E_ARG, "smx_ctx_subpixel_maps: the last smx_ctx_stereo_pair ran without sub-pixel");
    const size_t n = c->n, fb = n * sizeof(float);
    if (sub_l) SMX_HIP(c->sub.download(sub_l, fb));
    if (sub_r) SMX_HIP(hipMemcpy(sub_r, c->sub.as<float>() + n, fb, hipMemcpyDeviceToHost));
    if (sub_filled) SMX_HIP(c->subf.download(sub_filled, fb));
    return SMX_OK;
}

int smx_ctx_patchmatch_maps(smx_ctx* c, float* planes_l, float* planes_r, float* sub_l, float* sub_r, float* sub_filled) {
    SMX_ARG(c);
    if (int rc = ctx_check_device(c, "smx_ctx_patchmatch_maps")) return rc;
    if (!c->done.pm) return fail(SMX_E_ARG, "smx_ctx_patchmatch_maps: the last smx_ctx_stereo_pair ran without PatchMatch stereo");
    const size_t n = c->n, fb = n * sizeof(float);
    const float* pl = c->pm_planes.as<float>();
    const float* disp = c->pm_disp.as<float>();
    if (planes_l) SMX_HIP(hipMemcpy(planes_l, pl, 3 * fb, hipMemcpyDeviceToHost));
    if (planes_r) SMX_HIP(hipMemcpy(planes_r, pl + 3 * n, 3 * fb, hipMemcpyDeviceToHost));
    if (sub_l) SMX_HIP(hipMemcpy(sub_l, disp, fb, hipMemcpyDeviceToHost));
    if (sub_r) SMX_HIP(hipMemcpy(sub_r, disp + n, fb, hipMemcpyDeviceToHost));
    if (sub_filled) SMX_HIP(c->subf.download(sub_filled, fb));
    return SMX_OK;
}

// ---- test hooks (include/smx.h): what a stage holds on the device --------------------------------------------------------------
int smx_ctx_bp_held(const smx_ctx* c, size_t* bytes) {
    SMX_ARG(c && bytes);
    *bytes = c->bp_ws.p ? c->bp_ws.bytes : 0;
    return SMX_OK;
}

int smx_ctx_perm_held(const smx_ctx* c, size_t* bytes) {
    SMX_ARG(c && bytes);
    *bytes = c->perm_ws.p ? c->perm_ws.bytes : 0;
    return SMX_OK;
}

int smx_ctx_tree_held(const smx_ctx* c, size_t* bytes) {
    SMX_ARG(c && bytes);
    *bytes = 0;
    for (const DevBuf* b : {&c->tree_ws, &c->tree_dev}) *bytes += b->p ? b->bytes : 0;
    return SMX_OK;
}

int smx_ctx_pm_held(const smx_ctx* c, size_t* bytes) {
    SMX_ARG(c && bytes);
    *bytes = 0;
    for (const DevBuf* b : {&c->pm_planes, &c->pm_disp, &c->pm_ws}) *bytes += b->p ? b->bytes : 0;
    return SMX_OK;
}

int smx_ctx_cscale_held(const smx_ctx* c, int* levels, size_t* bytes) {
    SMX_ARG(c && levels && bytes);
    *levels = 0;
    *bytes = 0;
    for (const smx_ctx* k : c->cs_child) {
        if (!k) continue;
        ++*levels;
        for (const DevBuf* b : {&k->dL, &k->dR, &k->keys, &k->best, &k->map, &k->mean, &k->occ, &k->fil, &k->ws, &k->aggLR, &k->codes,
                                &k->adc_tab, &k->rgb, &k->mode_ws, &k->chunk_cost})
            *bytes += b->p ? b->bytes : 0;
    }
    return SMX_OK;
}

// ---- pipelined host-pointer entry ---------------------------------------------------------------------------------
// Pair k uses slot k % 2.  Three streams: uploads, the path, downloads; events chain a pair through them, so that the
// upload of pair k+1 and the download of pair k-1 run under the aggregation of pair k.
static int ctx_async_setup(smx_ctx* c) {
    if (c->st_up) return SMX_OK;
    const size_t n = c->n;
    for (hipStream_t* x : {&c->st_up, &c->st_dn}) SMX_HIP(hipStreamCreateWithFlags(x, hipStreamNonBlocking));
    for (smx_ctx::Slot& sl : c->slot) {
        SMX_HIP(sl.in.ensure(2 * n));
        SMX_HIP(sl.res.ensure(6 * n * sizeof(float)));
        SMX_HIP(sl.mean.ensure(2 * n));
        SMX_HIP(hipHostMalloc((void**)&sl.h_in, 2 * n, hipHostMallocDefault));
        SMX_HIP(hipHostMalloc((void**)&sl.h_out, 6 * n * sizeof(float) + 2 * n + 256, hipHostMallocDefault));
        for (hipEvent_t* e : {&sl.up, &sl.done, &sl.down}) SMX_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    return SMX_OK;
}

int smx_ctx_stereo_pair_async(smx_ctx* c, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr) {
    SMX_ARG(c && gray_l && gray_r);
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_stereo_pair_async"))) return rc;
    if (c->submitted - c->waited >= 2)
        return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: two pairs are in flight already (smx_ctx_wait takes the older one)");
    PairPlan need;
    char why[512];
    if (plan_pair(c->s, c->w, c->h, c->size_d, ENTRY_ASYNC, 0, dminl, dminr, false, false, false, &need, why, sizeof(why)))
        return fail(SMX_E_ARG, "%s", why);
    if ((rc = ctx_async_setup(c))) return rc;
    // no stage marks in the pipelined entry: pairs overlap on three streams, so "the stages of the last call" has no meaning
    // here, and an event record per stage is a bubble on the queue the pipeline exists to keep full
    TimingPause pause;
    const size_t n = c->n, fb = n * sizeof(float);
    smx_ctx::Slot& sl = c->slot[c->submitted & 1];
    // the caller's images into the slot's pinned staging: the caller's buffers are free again when this call returns
    memcpy(sl.h_in, gray_l, n);
    memcpy(sl.h_in + n, gray_r, n);
    uint8_t* dL = sl.in.as<uint8_t>(); uint8_t* dR = dL + n;
    SMX_HIP(hipMemcpyAsync(dL, sl.h_in, 2 * n, hipMemcpyHostToDevice, c->st_up));
    SMX_HIP(hipEventRecord(sl.up, c->st_up));
    SMX_HIP(hipStreamWaitEvent(c->st, sl.up, 0));
    float* r = sl.res.as<float>();                       // best_l best_r dmap_l dmap_r occlusion filled
    // (the plan of this entry has every opt-in stage off: the pair needs nothing beyond the eight planes)
    if ((rc = ctx_enqueue(c, {dL, dR, dminl, dminr}, need, {r, r + 2 * n, sl.mean.as<uint8_t>(), r + 4 * n, r + 5 * n})))
        return rc;
    // status word of this pair's aggregation (the next pair's launch clears it): behind the planes in the staging
    char* status_h = sl.h_out + 6 * fb + 2 * n;
    SMX_HIP(hipMemcpyAsync(status_h, (const char*)align_up((size_t)c->ws.p, 256), sizeof(unsigned), hipMemcpyDeviceToHost, c->st));
    SMX_HIP(hipEventRecord(sl.done, c->st));
    SMX_HIP(hipStreamWaitEvent(c->st_dn, sl.done, 0));
    SMX_HIP(hipMemcpyAsync(sl.h_out, r, 6 * fb, hipMemcpyDeviceToHost, c->st_dn));
    SMX_HIP(hipMemcpyAsync(sl.h_out + 6 * fb, sl.mean.p, 2 * n, hipMemcpyDeviceToHost, c->st_dn));
    SMX_HIP(hipEventRecord(sl.down, c->st_dn));
    ++c->submitted;
    return SMX_OK;
}

int smx_ctx_wait(smx_ctx* c, smx_pair_out* staged, const smx_pair_out* copy_to) {
    SMX_ARG(c);
    if (c->submitted == c->waited) return fail(SMX_E_ARG, "smx_ctx_wait: no pair in flight");
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_wait"))) return rc;
    smx_ctx::Slot& sl = c->slot[c->waited & 1];
    SMX_HIP(hipEventSynchronize(sl.down));
    ++c->waited;
    const size_t n = c->n, fb = n * sizeof(float);
    float* f = (float*)sl.h_out;
    uint8_t* m = (uint8_t*)(sl.h_out + 6 * fb);
    const smx_pair_out v = {f, f + n, f + 2 * n, f + 3 * n, m, m + n, f + 4 * n, f + 5 * n};     // (no volumes)
    if (staged) *staged = v;
    if (copy_to) {
        const auto to = pair_planes(*copy_to, c->size_d), from = pair_planes(v, c->size_d);
        for (size_t i = 0; i < to.size(); ++i)
            if (to[i].p && from[i].p) memcpy(to[i].p, from[i].p, n * from[i].elem);
    }
    unsigned status = 0;
    memcpy(&status, sl.h_out + 6 * fb + 2 * n, sizeof(status));
    return agg_status_error(status);
}

int smx_stereo_pair(const smx_params* p, const uint8_t* gray_l, const uint8_t* gray_r, int w, int h,
                    int size_d, int dminl, int dminr, const smx_pair_out* out) {
    SMX_ARG(p && gray_l && gray_r && out && w >= 2 && h >= 1 && size_d >= 1);
    smx_ctx* c = nullptr;
    if (int rc = smx_create(p, w, h, size_d, &c)) return rc;
    const int rc = smx_ctx_stereo_pair(c, gray_l, gray_r, dminl, dminr, out);
    (void)smx_destroy(c);
    return rc;
}

}  // extern "C"
