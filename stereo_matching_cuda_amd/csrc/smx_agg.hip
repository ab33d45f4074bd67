// smx_agg.hip -- host side of the aggregation (smx_agg.h): the gates of the two walkers, the workspace layouts, and the
// orchestration of one call.  Fused: guidance, then per chunk of slices a walker launch and a WTA pass.  Multi-kernel: per view
// guidance, then per chunk the passes of the reference's slice loop.  No kernel lives here: the comb walker's are in
// smx_agg_v5.hip, the ring walker's and the guidance kernels in smx_agg_v4.hip, the multi-kernel path's in smx_kernels.hip.
#include <string.h>

#include "smx_agg.h"
#include "smx_agg_v4.h"
#include "smx_agg_v5.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {

// =============================================================================================
// which aggregation a call runs
// =============================================================================================
// Both walkers build the cost of a partner outside the image from the sentinel cell (60000, 60000) of k_v4_guid_rows and rely
// on min(|d|, threshold) saturating to the threshold there, so that the cost is the border constant of costVolume.cu:184.  In
// the ring walker's f32 differences the nearest a pixel value (0 .. 255) and a derivative (multiples of 0.5 in [-127.5, 127.5])
// come to the sentinel is |255 - 60000| = 59745 and |127.5 - 60000| = 59872.5: larger thresholds would not saturate (the comb
// walker's bounds, in packed halves, are tighter: v5_supported).  The multi-kernel path uses the border constant itself.
constexpr int RING_TH_COLOR_MAX = 59745, RING_TH_GRAD_MAX = 59872;

static bool ring_applies(const smx_params* p, bool use_cost) {
    return v4_supported(p) && (use_cost || (p->th_color <= RING_TH_COLOR_MAX && p->th_grad <= RING_TH_GRAD_MAX));
}

// The comb walker (smx_agg_v5.hip) serves radius 9 with eps >= 1; with costs built from the images, default-like cost
// parameters (v5_supported); with materialised cost volumes, planes of at least one 16-byte quad (the kernel checks the values).
// It addresses both image planes, the guidance planes and their comb-ordered copies through ONE buffer descriptor with 32-bit
// offsets, 0x80000000 marking "outside": the whole region must stay below 2 GiB.
static bool v5_applies(const smx_params* p, int w, int h, int nviews, bool use_cost) {
    return v5_fix_bytes(w, h, nviews) < 0x80000000ull &&
           (use_cost ? v5_supported_cost(p) && (size_t)w * h >= 4 : v5_supported(p));
}

int agg_path_for(const smx_params* p, int w, int h, int nviews, bool use_cost, int forced, const char** why) {
    *why = nullptr;
    if (forced == 1) return 1;
    if (!ring_applies(p, use_cost)) {
        if (forced == 0) return 1;
        *why = !v4_supported(p) ? "radius > 9"
                                : "th_color > 59745 or th_grad > 59872 (the sentinel cell of an out-of-range partner would not "
                                  "saturate the truncation: only the multi-kernel path gives the border cost there)";
        return 0;
    }
    const bool comb = v5_applies(p, w, h, nviews, use_cost);
    if (forced == 5 && !comb) {
        *why = "the comb walker does not apply (radius 9, eps in [1, 1e30), default-like cost parameters where the costs are "
               "built from the images -- thresholds exact in fp16, th_color <= 59744, th_grad <= 59872 --, planes within "
               "its 2 GiB descriptor)";
        return 0;
    }
    if (forced == 3) return 2;
    if (forced == 4) return 4;
    return comb ? 5 : 2;
}

// =============================================================================================
// the workspace of the fused aggregation
// =============================================================================================
static size_t agg_ctrl_bytes(int K, size_t nsv) { return align_up(AGG_CTRL_BYTES + nsv * K * sizeof(unsigned), 256); }

AggLayout agg_layout(int w, int h, int radius, int nviews, bool comb, bool fallback, bool own_q, int chunk) {
    AggLayout L;
    memset(&L, 0, sizeof(L));
    L.comb = comb; L.fallback = fallback; L.own_q = own_q;
    L.nviews = nviews; L.chunk = chunk;
    L.K4 = v4::strips(w, radius); L.NI4 = v4::bands(h, radius);
    L.K = comb ? v5::strips(w) : L.K4;
    L.NI = comb ? v5::bands(h) : L.NI4;
    // records and flags are shared by the two walkers of a call with a queued fall-back: the larger of each
    const size_t hand4 = v4::sv_hand_floats(h, radius), hand = comb ? v5::sv_hand_floats(h) : hand4;
    L.hand_sv = fallback && hand4 > hand ? hand4 : hand;
    L.K_flags = fallback && L.K4 > L.K ? L.K4 : L.K;
    L.plane = (size_t)w * h;
    L.qplane = comb && own_q ? v5::q_plane_floats(w, h) : L.plane;
    L.q_slice = own_q ? align_up(L.qplane * 4, 256) : 0;

    size_t at = 0;
    auto region = [&at](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
    L.status = region(256);
    for (int i = 0; i < 2; ++i) L.fg[i] = region((size_t)(w + 2 * v4::PADX) * h * 4);      // (half2 = 4 B per pixel)
    for (int v = 0; v < nviews; ++v) L.guid[v] = region(L.plane * 8);
    // (band-major, smx_agg_v5.h: 5 NI row pairs of 16 B per lane; per band 16 B + 4 B per lane)
    const size_t permb = (size_t)v5::strips(w) * v5::bands(h) * v5::CLP;
    if (comb)
        for (int v = 0; v < nviews; ++v) {
            L.g1p[v] = region(permb * 5 * 16);
            L.i2p[v] = region(permb * 20);
        }
    L.fix_end = at;
    for (int v = 0; v < nviews; ++v)
        for (int i = 0; i < 2; ++i) L.scratch[v][i] = region(L.plane * 4);
    L.chunk_begin = at;
    const size_t nsv = (size_t)chunk * nviews;
    if (own_q)
        for (int v = 0; v < nviews; ++v) L.q[v] = region(chunk * L.q_slice);
    L.hand = region(nsv * L.hand_sv * 4);
    L.ctrl_bytes = agg_ctrl_bytes(L.K_flags, nsv);
    L.ctrl = region(L.ctrl_bytes);
    L.end = at;
    return L;
}

size_t v5_fix_bytes(int w, int h, int nviews) {
    const AggLayout L = agg_layout(w, h, v4::RMAX, nviews, true, false, true, 0);
    return L.fix_end - L.fg[0];
}

// the slices of a chunk are fitted with this much kept back: the round-ups of the chunk's regions and the ticket block
constexpr size_t FIT_RESERVE = 8 * 256 + AGG_CTRL_BYTES;

// What smx_agg_workspace_bytes* promise covers every call on a shape: the layout of one view at radius 9 on the comb walker with
// the queued fall-back (the larger q plane, records and strip count of the two walkers; both image planes, although a pair
// needs them once), its control block sized for the flags of both views of a pair, and
constexpr size_t WS_COMB_COPY_SLACK = 2 * 256;    // a round-up for each of the two comb-ordered copies
constexpr size_t WS_SLACK = 16 * 256;             // what agg_plan cannot use: up to 255 B in front of the 256-byte boundary + FIT_RESERVE
static_assert(WS_SLACK >= 255 + FIT_RESERVE, "a workspace sized for n slices holds n slices");
size_t agg_workspace_bytes(int w, int h, int nslices) {
    const AggLayout L = agg_layout(w, h, v4::RMAX, 1, true, true, true, nslices);
    return L.ctrl + agg_ctrl_bytes(L.K_flags, 2 * (size_t)nslices) + WS_COMB_COPY_SLACK + WS_SLACK;
}

int agg_plan(const smx_params* p, int w, int h, int nviews, bool use_cost, bool own_q, const AggOpts& opt, size_t ws_bytes,
             size_t lost, int total, AggLayout* L) {
    // The comb walker serves the hot case: radius 9, exact mode.  opt.walker: 0 = choose, 4 = the ring walker.  Both share the
    // orchestration: image planes, guidance statistics, chunking, WTA pass; only the strip / band geometry and the records differ.
    // Materialised cost volumes (the reference's calling convention, guidedFilter.cu:198-200) run on the comb walker too
    // (round 5): its cost wave loads the costs and CHECKS them -- +0 or a normal number in [2^-60, 2^60] is what its exactness
    // argument covers.  A violation cannot come back to the host of an asynchronous call, so the ring walker, which takes
    // any input, is queued behind it with a device-side gate (v4::Args::gate): it does nothing unless the comb walker raised the
    // second status word, and the two WTA passes are gated the other way round.  Cost: two empty launches and a memset.
    const bool comb = opt.walker != 4 && v5_applies(p, w, h, nviews, use_cost);
    const bool fallback = comb && use_cost;
    // (the entry points' decision once more: neither walker runs where agg_path_for would not send the call to it)
    const char* why = nullptr;
    if (!agg_path_for(p, w, h, nviews, use_cost, opt.walker == 5 ? 5 : 3, &why)) return fail(SMX_E_ARG, "aggregate_fused: %s", why);
    // every plane is addressed through 32-bit buffer offsets, with 0x80000000 as "outside the image"
    if ((size_t)h * ((size_t)w + 2 * v4::PADX) * 8 >= 0x80000000ull)
        return fail(SMX_E_ARG, "aggregate_fused: an image plane of %d x %d exceeds 2 GiB", w, h);
    const size_t avail = ws_bytes > lost ? ws_bytes - lost : 0;
    *L = agg_layout(w, h, p->radius, nviews, comb, fallback, own_q, 0);
    if (L->fg[0] > avail) return fail(SMX_E_WS, "aggregate_fused: workspace too small");
    // per slice-view: q plane (unless the caller's volume is written directly) + records + flags
    const size_t per_sv = L->q_slice + L->hand_sv * 4 + (size_t)L->K_flags * sizeof(unsigned);
    const size_t rest = avail > L->chunk_begin ? avail - L->chunk_begin : 0;
    const size_t fit = rest > FIT_RESERVE ? (rest - FIT_RESERVE) / (per_sv * nviews) : 0;
    if (L->chunk_begin > avail || (fit < 1 && total > 0))
        return fail(SMX_E_WS, "aggregate_fused: workspace %zu B too small (need >= %zu B per view)", ws_bytes,
                    agg_workspace_bytes(w, h, 1));
    int chunk = fit > (size_t)total ? total : (int)fit;
    if (opt.max_chunk > 0 && chunk > opt.max_chunk) chunk = opt.max_chunk;
    if (chunk < 1) chunk = 1;
    *L = agg_layout(w, h, p->radius, nviews, comb, fallback, own_q, chunk);
    if (L->end > avail) return fail(SMX_E_WS, "aggregate_fused: workspace carve overflow");
    return SMX_OK;
}

int agg_read_status(const void* d_ws, unsigned* out, int nwords) {
    const char* base = (const char*)align_up((size_t)d_ws, 256);
    SMX_HIP(hipMemcpy(out, base, sizeof(unsigned) * (size_t)nwords, hipMemcpyDeviceToHost));
    return SMX_OK;
}

// =============================================================================================
// one fused call
// =============================================================================================
// the comb walker's arguments for the chunk the ring walker's `a` describes
static v5::Args comb_args(const v4::Args& a, const AggLayout& L, char* base, bool use_cost, bool fast) {
    v5::Args b;
    memset(&b, 0, sizeof(b));
    b.fix = base + L.fg[0];
    b.fix_bytes = L.fix_end - L.fg[0];
    for (int v = 0; v < 2; ++v) {
        const int vv = v < L.nviews ? v : 0;
        b.o_fg[v] = (unsigned)(L.fg[v] - L.fg[0]);
        b.o_g1p[v] = (unsigned)(L.g1p[vv] - L.fg[0]);
        b.o_i2p[v] = (unsigned)(L.i2p[vv] - L.fg[0]);
        b.q[v] = a.v[vv].q;
        b.d0[v] = a.v[vv].d0;
        b.cost[v] = a.v[vv].cost;
    }
    b.w = a.w; b.h = a.h; b.K = L.K; b.NI = L.NI;
    b.P = v5::period(a.h, L.K);
    b.nslices = a.nslices; b.nsv = a.nsv; b.nitems = a.nitems;
    b.hand = (float*)a.hand; b.flags = a.flags; b.ticket = a.ticket; b.status = a.status;
    b.src_cost = use_cost ? 1 : 0;
    b.cost_plane = L.plane;
    b.bad = a.status + 1;
    b.cc = a.cc;
    const _Float16 hc = (_Float16)a.cc.th_color, hg = (_Float16)a.cc.th_grad;
    unsigned short uc, ug;
    memcpy(&uc, &hc, 2); memcpy(&ug, &hg, 2);
    b.th2 = (unsigned)uc | ((unsigned)ug << 16);
    b.fast = fast ? 1 : 0;
    // Role priorities (smx_agg_v5.hip PRIO_*) only while the launch's q planes stay below 6 GB.  Measured in rounds 4
    // and 5 (profiles/r05_prio_*): worth 2-7 % on KITTI geometry up to 1 500 slices (5.7 GB of q), on Motorcycle / 4K
    // geometry with few slices and on every aspect ratio at KITTI's volume; 0.4-4.8 % slower on 4K (34 GB of q per
    // launch), and -3.8 %, +3.0 % and -1.7 % on Motorcycle (15 GB) on three boxes.  The losing case has identical
    // instruction counts but vector-memory operations 32 % longer in flight (profiles/r05_prio_pmc_motorcycle.txt);
    // its cause is not established, so the rule follows the variable the effect follows: the q bytes of the launch.
    constexpr double PRIO_MAX_Q_BYTES = 6e9;
    const double q_bytes = (double)a.nsv * (double)L.qplane * 4.0;
    b.prio = q_bytes < PRIO_MAX_Q_BYTES ? 1 : 0;
    b.qperm = L.own_q ? 1 : 0;
    b.q_plane = L.qplane;
    return b;
}

// (dev / test hook, smx_debug_set_guidance_path: 0 = choose, 1 = the comb walker's guidance in three launches whatever the height)
static thread_local int g_guid_path = 0;
static thread_local int g_last_guid_bw = -1;      // the last fused call of this thread: columns per guidance block, 0 = three launches

// Image planes and guidance statistics of the call (guidedFilter.cu:58-123): (mean_I, 1/(var_I + eps)), the optional u8 mean
// image, the comb walker's comb-ordered copies.  Two launches on the comb-walker path where a column block's integral images
// fit the LDS (v5::guid_block_width: row prefixes, then k_v5_guid_block), else three (row prefixes, column prefixes,
// statistics).  *out: the planes the walkers read; *launches: how many it took.
static int guidance(const AggLayout& L, char* base, const AggCall& c, v4::Guidance* out, int* launches) {
    const int nviews = L.nviews, w = c.w, h = c.h;
    const smx_params* const p = c.p;
    hipStream_t st = c.st;
    v4::Guidance& g = *out;
    memset(&g, 0, sizeof(g));
    g.I[0] = c.guide[0];
    g.I[1] = nviews == 2 ? c.guide[1] : c.other[0];
    for (int i = 0; i < 2; ++i) g.FG[i] = (aggdev::fg_t*)(base + L.fg[i]);
    for (int v = 0; v < nviews; ++v) {
        g.S0[v] = (float*)(base + L.scratch[v][0]); g.S1[v] = (float*)(base + L.scratch[v][1]);
        g.G[v] = (aggdev::f2*)(base + L.guid[v]);
        g.mean_u8[v] = c.mean_u8[v];
    }
    // (the status words and the first chunk's control block are cleared here: no memset in front of the first walker)
    g.zero[0] = (unsigned*)(base + L.status); g.nzero[0] = 64;
    g.zero[1] = (unsigned*)(base + L.ctrl); g.nzero[1] = (unsigned)(L.ctrl_bytes / 4);
    const int bw = L.comb && g_guid_path != 1 ? v5::guid_block_width(h) : 0;
    g_last_guid_bw = bw;
    *launches = bw ? 2 : 3;
    int rc = v4_guidance_launch(g, nviews, w, h, p->radius, p->eps, !L.comb, bw == 0, st);
    if (rc || !L.comb) return rc;
    // (the comb walker's planes: the statistics are evaluated where the comb-ordered copy is written, and G / the u8
    // mean leave from there too -- one launch and one round trip of G less than finish + permute)
    aggdev::f2* g1p[2] = {nullptr, nullptr};
    unsigned* i2p[2] = {nullptr, nullptr};
    for (int v = 0; v < nviews; ++v) { g1p[v] = (aggdev::f2*)(base + L.g1p[v]); i2p[v] = (unsigned*)(base + L.i2p[v]); }
    if (bw) return v5_guid_block_launch(bw, nviews, g.S0, g.S1, g.G, g.mean_u8, g.FG, g1p, i2p, w, h, p->eps, st);
    return v5_perm_launch(nviews, g.S0, g.S1, g.G, g.mean_u8, g.FG, g1p, i2p, w, h, p->eps, st);
}

static int aggregate_fused(const AggCall& c, const AggOpts& opt, AggInfo* info) {
    const smx_params* const p = c.p;
    const int nviews = c.nviews, w = c.w, h = c.h, s_begin = c.s_begin, s_end = c.s_end;
    hipStream_t st = c.st;
    const bool use_cost = c.cost[0] != nullptr;
    const bool own_q = !c.agg[0];
    float* const* const d_nbr = c.nbr[0] ? c.nbr : nullptr;
    float* const* const d_uq = c.uq[0] ? c.uq : nullptr;
    char* const base = (char*)align_up((size_t)c.ws, 256);
    AggLayout L;
    int rc = agg_plan(p, w, h, nviews, use_cost, own_q, opt, c.ws_bytes, (size_t)(base - (char*)c.ws), s_end - s_begin, &L);
    if (rc) return rc;
    info->walker_used = L.comb ? 5 : 4;
    info->chunk = L.chunk;
    if (opt.keys_fresh && s_end <= s_begin) {
        // nothing to aggregate: the promise "the call presets the keys" still holds
        for (int v = 0; v < nviews; ++v)
            if ((rc = launch_init_keys(c.keys[v], (int64_t)w * h, st))) return rc;
    }
    unsigned* const status = (unsigned*)(base + L.status);
    char* const ctrl = base + L.ctrl;
    v4::Guidance g;
    int nl = 0;
    if ((rc = guidance(L, base, c, &g, &nl))) return rc;
    stage_mark(ST_GUIDANCE, st);

    v4::Args a0;
    memset(&a0, 0, sizeof(a0));
    a0.w = w; a0.h = h; a0.R = p->radius; a0.K = L.K; a0.NI = L.NI;
    a0.cc = make_cost_const(p);
    for (int v = 0; v < nviews; ++v) {
        a0.v[v].FG1 = g.FG[v]; a0.v[v].FG2 = g.FG[v ^ 1];
        a0.v[v].guid = g.G[v];
    }
    a0.hand = (aggdev::f2*)(base + L.hand);
    a0.ticket = (unsigned*)ctrl; a0.status = status;
    a0.flags = (unsigned*)(ctrl + AGG_CTRL_BYTES);
    const unsigned* const fell_back = L.fallback ? status + 1 : nullptr;     // raised by the comb walker: the ring walker's results count
    for (int s0 = s_begin; s0 < s_end; s0 += L.chunk) {
        const int cnt = (s_end - s0) < L.chunk ? (s_end - s0) : L.chunk;
        v4::Args a = a0;
        const float* q[2] = {nullptr, nullptr};
        for (int v = 0; v < nviews; ++v) {
            a.v[v].q = own_q ? (float*)(base + L.q[v]) : c.agg[v] + (size_t)(s0 - s_begin) * L.plane;   // (own planes: `qplane` floats apart)
            a.v[v].d0 = c.dmin[v] + s0;
            a.v[v].cost = use_cost ? c.cost[v] + (size_t)(s0 - s_begin) * L.plane : nullptr;
            q[v] = a.v[v].q;
        }
        a.nslices = cnt; a.nsv = cnt * nviews;
        a.nitems = a.nsv * L.K;
        const size_t ctrl_bytes = agg_ctrl_bytes(L.K_flags, a.nsv);
        if (s0 != s_begin) SMX_HIP(hipMemsetAsync(ctrl, 0, ctrl_bytes, st));   // (first chunk: cleared by k_v4_guid_rows)
        if (L.comb) {
            rc = v5_launch(comb_args(a, L, base, use_cost, opt.fast), st);
            if (!rc && L.fallback) {
                // the queued ring walker (does nothing unless status[1] was raised): its own geometry, fresh tickets and flags
                SMX_HIP(hipMemsetAsync(ctrl, 0, ctrl_bytes, st));
                v4::Args a4 = a;
                a4.K = L.K4; a4.NI = L.NI4;
                a4.nitems = a4.nsv * L.K4;
                a4.gate = fell_back;
                rc = v4_walk_launch(a4, true, opt.fast, st);
                nl += 2;
            }
        } else rc = v4_walk_launch(a, use_cost, opt.fast, st);
        if (rc) return rc;
        ++info->walker_launches;
        stage_mark(ST_WALK, st);
        // (opt.keys_fresh: the caller's keys hold nothing yet -- the first WTA pass of the call starts from the identity instead
        // of loading them, which saves the smx_dev_init_keys launch in front of the call; with the gated pair of passes of a
        // queued fall-back exactly one of the two runs, so both may take the flag)
        const bool fresh = opt.keys_fresh && s0 == s_begin;
        // (d_nbr / d_uq: the same passes that also keep the winners' neighbours, smx_common.h nbr_merge, and their second-best
        // cost, WtaRunUq; of the gated pair exactly one runs, so the state is advanced once)
        // over the planes of the walker that ran (smx_wta.h: runs iff gate == NULL || (*gate != 0) == gate_nonzero) ...
        const bool comb_q = L.comb && own_q;
        rc = wta_launch(comb_q ? WTA_COMB : WTA_NATURAL, nviews, q, c.keys, d_nbr, d_uq, w, h, L.qplane, cnt, s0,
                        comb_q ? fell_back : nullptr, 0, fresh, st);
        if (!rc && comb_q && L.fallback) {
            // ... and over the ring walker's planes ([slice][h][w] at the start of the same buffers), if it ran
            rc = wta_launch(WTA_NATURAL, nviews, q, c.keys, d_nbr, d_uq, w, h, L.plane, cnt, s0, fell_back, 1, fresh, st);
            ++nl;
        }
        if (rc) return rc;
        stage_mark(ST_WTA, st);
        nl += s0 != s_begin ? 3 : 2;
    }
    info->launches = nl;
    return SMX_OK;
}

// =============================================================================================
// the multi-kernel path: its workspace, one call
// =============================================================================================
MultiLayout multi_layout(int w, int h, bool use_cost, int chunk) {
    MultiLayout L;
    memset(&L, 0, sizeof(L));
    L.chunk = chunk;
    L.volumes = use_cost ? 4 : 5;
    size_t at = 0;
    auto region = [&at](size_t bytes) { const size_t o = at; at += align_up(bytes, 256); return o; };
    const size_t plane = (size_t)w * h * sizeof(float);
    L.status = region(256);
    for (size_t* o : {&L.im, &L.mean_im, &L.cinv, &L.g0, &L.g1}) *o = region(plane);
    L.chunk_begin = at;
    for (size_t* o : {&L.T0, &L.T1, &L.A, &L.B}) *o = region(chunk * plane);
    if (!use_cost) L.C = region(chunk * plane);
    L.end = at;
    return L;
}

// What smx_agg_workspace_bytes promises for this path: costs built from the images, every slice's planes rounded up on their
// own (never less than the layout of nslices slices), and the up to 255 B in front of the workspace's 256-byte boundary.
size_t multi_workspace_bytes(int w, int h, int nslices) {
    const MultiLayout L = multi_layout(w, h, false, 1);
    return L.end + (size_t)(nslices - 1) * (L.end - L.chunk_begin) + 256;
}

int multi_plan(const char* who, int w, int h, bool use_cost, size_t ws_bytes, size_t lost, int total, MultiLayout* L) {
    const size_t avail = ws_bytes > lost ? ws_bytes - lost : 0;
    // (every call needs the room of one slice whose costs are built from the images, also where they are materialised)
    if (multi_layout(w, h, false, 1).end > avail)
        return fail(SMX_E_WS, "%s: workspace %zu B < %zu B needed for one slice", who, ws_bytes, multi_workspace_bytes(w, h, 1));
    // the largest chunk, of at most `total` slices, whose layout ends inside the workspace: from what would fit unrounded
    *L = multi_layout(w, h, use_cost, 1);
    const size_t fit = (avail - L->chunk_begin) / L->volumes / ((size_t)w * h * sizeof(float));
    int chunk = fit > (size_t)total ? total : (int)fit;
    if (chunk < 1) chunk = 1;
    while (chunk > 1 && multi_layout(w, h, use_cost, chunk).end > avail) --chunk;
    *L = multi_layout(w, h, use_cost, chunk);
    return SMX_OK;
}

// guidedFilter.cu:58-238 for every view of the call, one after the other in the same planes: the guidance statistics in three
// launches, then `chunk` slices per pass of the slice loop.  The WTA is folded into the last launch of a pass.
static int aggregate_multi(const AggCall& c, const AggOpts& opt, AggInfo* info) {
    const smx_params* const p = c.p;
    const int w = c.w, h = c.h;
    hipStream_t st = c.st;
    const int64_t n = (int64_t)w * h;
    char* const base = (char*)align_up((size_t)c.ws, 256);
    MultiLayout L;
    int rc = multi_plan(c.who, w, h, c.cost[0] != nullptr, c.ws_bytes, (size_t)(base - (char*)c.ws), c.s_end - c.s_begin, &L);
    if (rc) return rc;
    info->chunk = L.chunk;
    float* const im = (float*)(base + L.im);
    float* const mean_im = (float*)(base + L.mean_im);
    float* const cinv = (float*)(base + L.cinv);
    float* const g0 = (float*)(base + L.g0);
    float* const g1 = (float*)(base + L.g1);
    float* const T0 = (float*)(base + L.T0);
    float* const T1 = (float*)(base + L.T1);
    float* const A = (float*)(base + L.A);
    float* const B = (float*)(base + L.B);
    float* const C = L.C ? (float*)(base + L.C) : nullptr;
    for (int v = 0; v < c.nviews; ++v) {
        if (opt.keys_fresh && (rc = launch_init_keys(c.keys[v], n, st))) return rc;
        SMX_HIP(hipMemsetAsync(base + L.status, 0, 256, st));
        // guidance statistics (guidedFilter.cu:58-123)
        if ((rc = launch_guid_prep(c.guide[v], im, g1, n, st))) return rc;
        if ((rc = launch_integral(2, im, g1, g0, g1, w, h, 1, st))) return rc;
        if ((rc = launch_guid_finish(p, g0, g1, mean_im, cinv, c.mean_u8[v], w, h, st))) return rc;
        info->launches += 4;
        stage_mark(ST_GUIDANCE, st);
        // slice loop (guidedFilter.cu:171-238)
        for (int s0 = c.s_begin; s0 < c.s_end; s0 += L.chunk) {
            const int cnt = (c.s_end - s0) < L.chunk ? (c.s_end - s0) : L.chunk;
            const float* cost = c.cost[v] ? c.cost[v] + (int64_t)(s0 - c.s_begin) * n : C;
            if (!c.cost[v]) {
                if ((rc = launch_cost(p, c.guide[v], c.other[v], C, w, h, c.dmin[v] + s0, cnt, st))) return rc;
                ++info->launches;
            }
            if ((rc = launch_integral(1, cost, im, T0, T1, w, h, cnt, st))) return rc;
            if ((rc = launch_ab(p, T0, T1, mean_im, cinv, A, B, w, h, cnt, st))) return rc;
            if ((rc = launch_integral(2, A, B, A, B, w, h, cnt, st))) return rc;
            float* agg = c.agg[v] ? c.agg[v] + (int64_t)(s0 - c.s_begin) * n : nullptr;
            if ((rc = launch_q_wta(p, A, B, im, c.keys[v], c.nbr[v], c.uq[v], agg, w, h, cnt, s0, st))) return rc;
            info->launches += 6;
            stage_mark(ST_WALK, st);
        }
    }
    return SMX_OK;
}

// =============================================================================================
// the one dispatch
// =============================================================================================
int aggregate(const AggCall& c, int forced, const AggOpts& opt, AggInfo* info) {
    const bool use_cost = c.cost[0] != nullptr;
    if (c.nviews == 2 && use_cost != (c.cost[1] != nullptr))
        return fail(SMX_E_ARG, "%s: both views need a cost volume or none", c.who);
    const char* why = nullptr;
    const int path = agg_path_for(c.p, c.w, c.h, c.nviews, use_cost, forced, &why);
    if (!path) return fail(SMX_E_ARG, "%s: fused path %d forced but %s", c.who, forced, why);
    AggInfo mine;
    if (!info) info = &mine;
    *info = AggInfo();
    info->path = path;
    if (path == 1) return aggregate_multi(c, opt, info);
    AggOpts o = opt;
    o.take_path(path);
    return aggregate_fused(c, o, info);
}

}  // namespace smx

// (dev / test hooks, not in smx.h: the guidance launches of the calling thread's fused aggregations on the comb-walker path --
// 0 = choose (two launches where v5::guid_block_width(h) > 0), 1 = three launches whatever the height; what the thread's last
// fused call ran with: *bw = columns per guidance block, 0 = three launches, -1 = no call yet; and the choice itself, pure host
// arithmetic: the block width for h rows, 0 = none fits, and the LDS bytes of that block)
extern "C" __attribute__((visibility("default"))) int smx_debug_set_guidance_path(int path) {
    if (path < 0 || path > 1) return smx::fail(SMX_E_ARG, "smx_debug_set_guidance_path: path must be 0 or 1");
    smx::g_guid_path = path;
    return SMX_OK;
}
extern "C" __attribute__((visibility("default"))) int smx_debug_last_guidance_block(int* bw) {
    SMX_ARG(bw);
    *bw = smx::g_last_guid_bw;
    return SMX_OK;
}
extern "C" __attribute__((visibility("default"))) int smx_debug_guidance_block(int h, int* bw, uint64_t* lds_bytes) {
    SMX_ARG(h >= 1 && bw);
    *bw = smx::v5::guid_block_width(h);
    if (lds_bytes) *lds_bytes = *bw ? (uint64_t)smx::v5::guid_block_lds(h, *bw) : 0;
    return SMX_OK;
}
