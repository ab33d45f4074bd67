// smx_capi.hip -- the C-ABI of include/smx.h: the calling thread's state (last error, knobs, stage timing), the device-pointer
// entries with their argument checks and the smx_debug_* hooks.  The host-pointer wrappers (smx_host.hip) and the persistent
// context (smx_ctx.hip) reach the thread's state through smx_api.h only.  Every aggregation goes through run_aggregation.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "smx_api.h"
#include "smx_agg_v4.h"
#include "smx_agg_v5.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {

static thread_local std::string g_err;
static thread_local int g_timing = 0;        // 0 off, 1 the last call, 2 cumulative over calls
static thread_local int g_launches = 0;
static thread_local int g_marks_dropped = 0;
// Stage timing of the calling thread (smx_set_timing / smx_stage_times): a list of (stage, event) marks of the
// last timed call; the time between two consecutive marks belongs to the stage of the later one.  Events are taken
// from a pool per device (an event records on the device that was current when it was created).
struct StageTimer {
    struct Mark { int stage; hipEvent_t ev; };
    std::vector<Mark> marks;
    std::vector<std::vector<hipEvent_t>> pool;   // [device] -> events
    std::vector<size_t> used;                    // [device] -> events handed out for the current call
    void begin() { marks.clear(); for (auto& u : used) u = 0; }
    hipEvent_t get() {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return nullptr;
        if ((size_t)dev >= pool.size()) { pool.resize(dev + 1); used.resize(dev + 1, 0); }
        if (used[dev] == pool[dev].size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            pool[dev].push_back(e);
        }
        return pool[dev][used[dev]++];
    }
};
static thread_local StageTimer g_timer;
// Aggregation path of the calling thread's smx_dev_* / host-pointer calls (smx_set_agg_path); a persistent
// context carries its own (smx_ctx_set_agg_path).  0 auto, 1 multi-kernel, 2 fused (walker chosen by the call),
// 3 fused with the ring walker (smx_agg_v4.hip), 4 fused FAST (not bit-exact), 5 fused with the comb walker
// (smx_agg_v5.hip; an error where it does not apply)
static thread_local int g_agg_path = 0;
static thread_local int g_last_path = 0;
static thread_local int g_max_chunk = 0;     // smx_set_max_slices_per_launch
static thread_local int g_keys_fresh = 0;    // smx_set_keys_fresh
static thread_local AggInfo g_last_info;     // smx_last_agg_chunk: the last FUSED aggregation

// (smx_api.h)  A context call, too, takes keys_fresh and max_chunk from the CALLING thread, and smx_last_agg_chunk keeps
// describing the thread's last fused aggregation (smx.h), so a multi-kernel call leaves it alone.
int run_aggregation(const AggCall& c, int forced, bool accumulates) {
    AggOpts opt;
    opt.keys_fresh = g_keys_fresh != 0 && !accumulates;
    opt.max_chunk = g_max_chunk;
    AggInfo info;
    g_launches = 0;
    const int rc = aggregate(c, forced, opt, &info);
    if (rc) return rc;
    g_last_path = info.path;
    g_launches = info.launches;
    if (info.path != 1) g_last_info = info;
    return SMX_OK;
}

void stage_mark(int stage, hipStream_t st) {
    if (!g_timing) return;
    if (stage == ST_BEGIN && g_timing == 1) { g_timer.begin(); g_marks_dropped = 0; }
    if (g_timer.marks.size() >= 32768) { ++g_marks_dropped; return; }
    hipEvent_t e = g_timer.get();
    if (!e || hipEventRecord(e, st) != hipSuccess) return;
    g_timer.marks.push_back({stage, e});
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int thread_agg_path() { return g_agg_path; }
int thread_max_chunk() { return g_max_chunk; }
TimingPause::TimingPause() : saved(g_timing) { g_timing = 0; }
TimingPause::~TimingPause() { g_timing = saved; }
int agg_status_error(unsigned status) {
    if (status == 0) return SMX_OK;
    return fail(SMX_E_HIP, "fused aggregation: hand-off wait of work item %u timed out (results invalid)", status - 1);
}

bool subpix_mode_ok(int mode) { return mode == SMX_SUBPIX_PARABOLA || mode == SMX_SUBPIX_EQUIANGULAR; }
bool wmf_params_ok(const smx_wmf_params* p) {
    return p && p->radius >= 1 && p->radius <= 15 && isfinite(p->sigma_s) && p->sigma_s > 0 && isfinite(p->sigma_c) &&
           p->sigma_c > 0;
}
bool census_params_ok(const smx_census_params* p) { return p && p->rx >= 1 && p->rx <= 4 && p->ry >= 1 && p->ry <= 3 && p->th >= 1; }
bool zncc_params_ok(const smx_zncc_params* p) { return p && p->rx >= 1 && p->rx <= 4 && p->ry >= 1 && p->ry <= 4; }
bool adcensus_params_ok(const smx_adcensus_params* p) {
    return p && census_params_ok(&p->census) && isfinite(p->lambda_census) && p->lambda_census > 0 && p->lambda_census <= 1e6 &&
           isfinite(p->lambda_ad) && p->lambda_ad > 0 && p->lambda_ad <= 1e6 && isfinite(p->scale) && p->scale >= 0x1p-20 &&
           p->scale <= 0x1p20 && (p->colour == 0 || p->colour == 1);
}
bool uniq_ratio_ok(float ratio) { return isfinite(ratio) && ratio >= 0.0f; }
bool speckle_params_ok(const smx_speckle_params* p) { return p && p->max_size >= 0 && isfinite(p->max_diff) && p->max_diff >= 0.0f; }
bool sgm_params_ok(const smx_sgm_params* p) {
    return p && p->p1 >= 0 && p->p1 <= p->p2 && p->p2 <= 4095 && (p->paths == 4 || p->paths == 8);
}
bool scanline_params_ok(const smx_scanline_params* p) {
    return p && p->p1 >= 0 && p->p1 <= p->p2 && p->p2 <= 4095 && p->tau_so >= 1 && p->tau_so <= 256 && (p->paths == 4 || p->paths == 8);
}
bool bp_params_ok(const smx_bp_params* p) {
    return p && p->step >= 0 && p->step <= 4095 && p->trunc >= 0 && p->trunc <= 4095 && p->iterations >= 0 && p->iterations <= 64 &&
           p->levels >= 1 && p->levels <= 8 && isfinite(p->data_scale) && p->data_scale > 0;
}

}  // namespace smx

using namespace smx;

extern "C" {

void smx_default_params(smx_params* p) {
    if (!p) return;
    p->r_w = 0.299; p->g_w = 0.587; p->b_w = 0.0721;
    p->alpha = 0.9; p->th_color = 7; p->th_grad = 2;
    p->radius = 9; p->eps = 6.5025; p->d_lr = 0;
}

const char* smx_last_error(void) { return g_err.c_str(); }

const char* smx_version(void) { return "smx-hip gfx950 0.11 (sub-pixel disparity from the winner's neighbouring costs: smx_dev_subpixel_pair; weighted-median refinement of the filled map: smx_weighted_median; comb walker: items pipelined across tickets, q scratch in row pairs, cost volumes on the comb walker, row pairs outside the image reduced to their column sums; WTA winner in the float domain; guidance in two launches where a column block's integral images fit the LDS, else three; two 512-thread workgroups per CU)"; }

int smx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int64_t smx_pack_key(float cost, uint32_t slice) { return pack_key(cost, slice); }
void smx_unpack_key(int64_t key, float* cost, uint32_t* slice) {
    float c; uint32_t s;
    unpack_key(key, &c, &s);
    if (cost) *cost = c;
    if (slice) *slice = s;
}

int smx_set_timing(int mode) {
    if (mode < 0 || mode > 2) return fail(SMX_E_ARG, "smx_set_timing: mode must be 0, 1 or 2");
    g_timing = mode;
    g_timer.begin();
    g_marks_dropped = 0;
    return SMX_OK;
}

int smx_stage_times(smx_stage_ms* out) {
    SMX_ARG(out);
    memset(out, 0, sizeof(*out));
    if (g_timer.marks.size() < 2) return fail(SMX_E_ARG, "smx_stage_times: no timed call recorded (smx_set_timing(1) first)");
    SMX_HIP(hipEventSynchronize(g_timer.marks.back().ev));
    float acc[ST_COUNT] = {0};
    int calls = g_timer.marks.front().stage == ST_BEGIN ? 1 : 0;
    for (size_t i = 1; i < g_timer.marks.size(); ++i) {
        if (g_timer.marks[i].stage == ST_BEGIN) { ++calls; continue; }     // (the gap in front of a call is nobody's)
        float t = 0;
        SMX_HIP(hipEventElapsedTime(&t, g_timer.marks[i - 1].ev, g_timer.marks[i].ev));
        acc[g_timer.marks[i].stage] += t;
    }
    out->calls = calls;
    out->dropped = g_marks_dropped;
    out->upload = acc[ST_UPLOAD]; out->guidance = acc[ST_GUIDANCE]; out->aggregation = acc[ST_WALK];
    out->wta = acc[ST_WTA]; out->finish = acc[ST_FINISH]; out->download = acc[ST_DOWNLOAD];
    out->total = out->upload + out->guidance + out->aggregation + out->wta + out->finish + out->download;
    return SMX_OK;
}

int smx_last_agg_ms(float* ms, int* launches) {
    smx_stage_ms t;
    int rc = smx_stage_times(&t);
    if (rc) return rc;
    if (ms) *ms = t.guidance + t.aggregation + t.wta;
    if (launches) *launches = g_launches;
    return SMX_OK;
}

/* ------------------------------------------------------------------------------------------
 * device-pointer API
 * ---------------------------------------------------------------------------------------- */

int smx_dev_rgb_to_grayscale(const smx_params* p, const uint8_t* d_rgb, int64_t n, int channels,
                             uint8_t* d_gray, void* stream) {
    SMX_ARG(p && d_rgb && d_gray && n > 0 && channels >= 3);
    return launch_gray(p, d_rgb, n, channels, d_gray, (hipStream_t)stream);
}

int smx_dev_cost_volume(const smx_params* p, const uint8_t* d_i1, const uint8_t* d_i2, float* d_cost,
                        int w1, int w2, int h, int dmin, int s_begin, int s_end, void* stream) {
    SMX_ARG(p && d_i1 && d_i2 && d_cost);
    SMX_ARG(w1 >= 2 && h >= 1 && w1 == w2 && s_begin >= 0 && s_end >= s_begin);
    return launch_cost(p, d_i1, d_i2, d_cost, w1, h, dmin + s_begin, s_end - s_begin,
                       (hipStream_t)stream);
}

int smx_dev_integral(const float* d_in, float* d_out, int w, int h, int nplanes, void* stream) {
    SMX_ARG(d_in && d_out && w >= 1 && h >= 1 && nplanes >= 0);
    return launch_integral(0, d_in, nullptr, d_out, nullptr, w, h, nplanes, (hipStream_t)stream);
}

size_t smx_agg_workspace_bytes(int w, int h, int nslices) {
    if (w < 1 || h < 1 || nslices < 1) return 0;
    // whichever path the call runs: the multi-kernel one (five planes per slice in flight) or a fused walker
    const size_t m = multi_workspace_bytes(w, h, nslices), f = agg_workspace_bytes(w, h, nslices);
    return m > f ? m : f;
}

size_t smx_agg_workspace_bytes_for(const smx_params* p, int w, int h, int nslices) {
    if (!p || w < 1 || h < 1 || nslices < 1) return 0;
    // where a fused walker runs for costs built from the images (agg_path_for; forced paths aside: smx_set_agg_path(1) callers
    // size with smx_agg_workspace_bytes): image / guidance planes, per slice ONE q plane + the hand-off records
    const char* why = nullptr;
    if (agg_path_for(p, w, h, 2, false, 0, &why) != 1) return agg_workspace_bytes(w, h, nslices);
    return smx_agg_workspace_bytes(w, h, nslices);
}

int smx_set_agg_path(int path) {
    if (path < 0 || path > 5) return fail(SMX_E_ARG, "smx_set_agg_path: path must be 0 .. 5");
    g_agg_path = path;
    return SMX_OK;
}

int smx_last_agg_path(void) { return g_last_path; }

int smx_set_keys_fresh(int on) {
    g_keys_fresh = on ? 1 : 0;
    return SMX_OK;
}

int smx_set_max_slices_per_launch(int n) {
    if (n < 0) return fail(SMX_E_ARG, "smx_set_max_slices_per_launch: n must be >= 0 (0 = as many as the workspace holds)");
    g_max_chunk = n;
    return SMX_OK;
}

int smx_last_agg_chunk(int* slices_per_launch, int* walker_launches) {
    if (slices_per_launch) *slices_per_launch = g_last_info.chunk;
    if (walker_launches) *walker_launches = g_last_info.walker_launches;
    return SMX_OK;
}

// (dev / test hook, not in smx.h: the size of the region the comb walker addresses through one 32-bit-offset descriptor)
__attribute__((visibility("default"))) int smx_debug_v5_fix_bytes(int w, int h, int nviews, uint64_t* bytes) {
    SMX_ARG(bytes && w >= 2 && h >= 1 && (nviews == 1 || nviews == 2));
    *bytes = (uint64_t)v5_fix_bytes(w, h, nviews);
    return SMX_OK;
}

// (dev / test hook, not in smx.h: the aggregation a call with these arguments runs -- agg_path_for, the decision every entry
// takes: 1 multi-kernel, 2 ring walker, 4 FAST, 5 comb walker; SMX_E_ARG where the forced path does not apply)
__attribute__((visibility("default"))) int smx_debug_agg_path(const smx_params* p, int w, int h, int nviews, int use_cost,
                                                              int forced, int* path) {
    SMX_ARG(p && path && w >= 2 && h >= 1 && (nviews == 1 || nviews == 2) && forced >= 0 && forced <= 5 && p->radius >= 0);
    const char* why = nullptr;
    const int r = agg_path_for(p, w, h, nviews, use_cost != 0, forced, &why);
    if (!r) return fail(SMX_E_ARG, "smx_debug_agg_path: fused path %d forced but %s", forced, why);
    *path = r;
    return SMX_OK;
}

// (dev / test hook, not in smx.h: the slices per walker launch, or per pass of the multi-kernel path, of a call with these
// arguments -- agg_plan / multi_plan, the layout the call runs with -- on a workspace of ws_bytes that loses the worst case of
// 255 bytes to its 256-byte alignment; forced as for smx_debug_agg_path; SMX_E_WS where the workspace holds no slice; the
// thread's knobs are not applied)
__attribute__((visibility("default"))) int smx_debug_agg_chunk(const smx_params* p, int w, int h, int nviews, int use_cost,
                                                               int own_q, int forced, uint64_t ws_bytes, int slices, int* chunk) {
    SMX_ARG(p && chunk && w >= 2 && h >= 1 && (nviews == 1 || nviews == 2) && forced >= 0 && forced <= 5 && p->radius >= 0 && slices >= 0);
    const char* why = nullptr;
    const int path = agg_path_for(p, w, h, nviews, use_cost != 0, forced, &why);
    if (!path) return fail(SMX_E_ARG, "smx_debug_agg_chunk: fused path %d forced but %s", forced, why);
    AggOpts opt;
    opt.take_path(path);
    AggLayout L;
    MultiLayout M;
    const int rc = path == 1 ? multi_plan("smx_debug_agg_chunk", w, h, use_cost != 0, (size_t)ws_bytes, 255, slices, &M)
                             : agg_plan(p, w, h, nviews, use_cost != 0, own_q != 0, opt, (size_t)ws_bytes, 255, slices, &L);
    if (rc) return rc;
    *chunk = path == 1 ? M.chunk : L.chunk;
    return SMX_OK;
}

// (dev / test hook, not in smx.h: WtaRun, the float-domain winner of a run of ascending slices as the WTA kernels form it)
__attribute__((visibility("default"))) int smx_debug_wta_run(const float* q, int n, uint32_t slice0, int64_t* key) {
    SMX_ARG(q && key && n >= 0);
    WtaRun r;
    for (int i = 0; i < n; ++i) r.step(q[i], slice0 + (uint32_t)i);
    *key = r.key();
    return SMX_OK;
}

// (dev / test hook, not in smx.h: WtaRunUq over one chunk of ascending slices, resumed from key / state [sec, rest, last] and
// left there -- the pixel of the UQ passes on the host)
__attribute__((visibility("default"))) int smx_debug_uq_run(const float* q, int n, uint32_t slice0, int64_t* key, float* state) {
    SMX_ARG(q && key && state && n >= 0);
    WtaRunUq r;
    r.resume(*key, state[0], state[1], state[2]);
    for (int i = 0; i < n; ++i) r.step(q[i], slice0 + (uint32_t)i);
    *key = r.key();
    state[0] = r.sec; state[1] = r.rest; state[2] = r.last;
    return SMX_OK;
}

// (dev / test hook, not in smx.h: the uniqueness test of one pixel as the filter kernel forms it; returns 1 where rejected)
__attribute__((visibility("default"))) int smx_debug_uniq_test(int64_t key, float s, float ratio, float* margin) {
    SMX_ARG(margin);
    return uniq_rejects(key, s, ratio, margin) ? 1 : 0;
}

// (dev / test hook, not in smx.h: the comb walker's slot geometry for an image of h rows in K strips -- bands per item, the
// last stage-2 slot, the period between the starts of two items of a workgroup -- for tools/v5_protocol_sim.py)
__attribute__((visibility("default"))) int smx_debug_v5_period(int h, int K, int* bands, int* q_last, int* period) {
    SMX_ARG(h >= 1 && K >= 1);
    int b = 0, q = 0, pd = 0;
    v5_slots(h, K, &b, &q, &pd);
    if (bands) *bands = b;
    if (q_last) *q_last = q;
    if (period) *period = pd;
    return SMX_OK;
}

int smx_agg_geometry(int radius, int* strip_cols, int* band_rows, int* tile_cols) {
    int ow = v4::OW, bh = v4::BH;
    smx_params p;
    smx_default_params(&p);
    p.radius = radius;
    if (g_agg_path != 3 && g_agg_path != 4 && v5_supported(&p)) { ow = v5::OWS; bh = v5::BH; }   // the comb walker
    if (strip_cols) *strip_cols = ow;
    if (band_rows) *band_rows = bh;
    if (tile_cols) *tile_cols = ow + 2 * radius + 1;
    return SMX_OK;
}

int smx_dev_agg_status(const void* d_workspace) {
    SMX_ARG(d_workspace);
    unsigned st = 0;
    int rc = agg_read_status(d_workspace, &st, 1);
    return rc ? rc : agg_status_error(st);
}

int smx_dev_agg_fallback(const void* d_workspace, int* ring_walker_reran) {
    SMX_ARG(d_workspace && ring_walker_reran);
    unsigned st[2] = {0, 0};
    int rc = agg_read_status(d_workspace, st, 2);
    if (rc) return rc;
    *ring_walker_reran = st[1] != 0;
    return SMX_OK;
}

// The kernels are launched on the CURRENT device: a workspace that lives on another one is a caller bug
// that would otherwise fault on the GPU.
static int check_same_device(const void* d_ws, const char* who) {
    hipPointerAttribute_t a;
    int dev = -1;
    if (hipPointerGetAttributes(&a, d_ws) != hipSuccess) {
        (void)hipGetLastError();
        return SMX_OK;   // not a pointer the runtime knows (e.g. a sub-allocation it cannot resolve): let it through
    }
    SMX_HIP(hipGetDevice(&dev));
    if (a.type == hipMemoryTypeDevice && a.device != dev)
        return fail(SMX_E_ARG, "%s: workspace lives on device %d but the current device is %d "
                               "(hipSetDevice to the workspace's device before the call)", who, a.device, dev);
    return SMX_OK;
}

int smx_dev_init_keys(int64_t* d_keys, int64_t n, void* stream) {
    SMX_ARG(d_keys && n > 0);
    return launch_init_keys(d_keys, n, (hipStream_t)stream);
}

int smx_dev_init_wta(float* d_best, float* d_dmap, int64_t n, void* stream) {
    SMX_ARG(d_best && d_dmap && n > 0);
    return launch_init_wta(d_best, d_dmap, n, (hipStream_t)stream);
}

int smx_dev_apply_keys(const int64_t* d_keys, int64_t n, int dmin, float* d_best, float* d_dmap,
                       void* stream) {
    SMX_ARG(d_keys && d_best && d_dmap && n > 0);
    return launch_apply_keys(d_keys, n, dmin, d_best, d_dmap, (hipStream_t)stream);
}

int smx_dev_detect_occlusion(const smx_params* p, float* d_dL, const float* d_dR, int dOcclusion,
                             int w, int h, void* stream) {
    SMX_ARG(p && d_dL && d_dR && w >= 1 && h >= 1);
    return launch_detect_occlusion(p, d_dL, d_dR, dOcclusion, w, h, (hipStream_t)stream);
}

int smx_dev_fill_occlusion(float* d_disp, int w, int h, float vMin, void* stream) {
    SMX_ARG(d_disp && w >= 1 && h >= 1);
    return launch_fill_occlusion(d_disp, d_disp, w, h, vMin, (hipStream_t)stream);
}

// main.cu:112-155 behind the aggregation, both views, in three launches (presets + winning slices + copy of
// the left map; LR check; filling out of place) instead of the seven of the per-call sequence
int smx_dev_finish_pair(const smx_params* p, const int64_t* d_keys, int w, int h, int dminl, int dminr,
                        int dOcclusion, float vMin, float* d_best, float* d_dmap, float* d_occlusion,
                        float* d_filled, void* stream) {
    SMX_ARG(p && d_keys && d_best && d_dmap && d_occlusion && d_filled && w >= 1 && h >= 1);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)w * h;
    int rc;
    // one launch (a row per workgroup) where the row fits the LDS three times, else the three kernels
    if (finish_pair_row_supported(w) && d_filled != d_occlusion) {
        rc = launch_finish_pair_row(p, d_keys, w, h, dminl, dminr, dOcclusion, vMin, d_best, d_dmap, d_occlusion,
                                    d_filled, st);
    } else {
        if ((rc = launch_finish_keys(d_keys, n, dminl, dminr, d_best, d_dmap, d_occlusion, st))) return rc;
        if ((rc = launch_detect_occlusion(p, d_occlusion, d_dmap + n, dOcclusion, w, h, st))) return rc;
        rc = launch_fill_occlusion(d_occlusion, d_filled, w, h, vMin, st);
    }
    stage_mark(ST_FINISH, st);
    return rc;
}

// The tail of the five device entries: the kernels need the workspace on the current device; one timed call; the thread's path
static int dev_aggregate(const AggCall& c) {
    const int rc = check_same_device(c.ws, c.who);
    if (rc) return rc;
    stage_mark(ST_BEGIN, c.st);
    return run_aggregation(c, g_agg_path, false);
}

// smx_dev_aggregate_wta and, with d_nbr != NULL (the view's state planes, smx_common.h nbr_merge), its _nbr form
static int aggregate_view(const char* who, const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                          const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                          int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                          size_t workspace_bytes, float* d_nbr, void* stream) {
    SMX_ARG(p && d_guide && d_keys && d_workspace);
    SMX_ARG(d_cost || d_other);
    SMX_ARG(w >= 2 && h >= 1 && s_begin >= 0 && s_end >= s_begin && p->radius >= 0);
    const AggCall c = {who, p, 1, {d_guide}, {d_other}, {d_cost}, {dmin}, {d_keys}, {d_mean_u8}, {d_agg}, {d_nbr}, {nullptr},
                       w, h, s_begin, s_end, d_workspace, workspace_bytes, (hipStream_t)stream};
    return dev_aggregate(c);
}

int smx_dev_aggregate_wta(const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                          const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                          int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
    return aggregate_view("smx_dev_aggregate_wta", p, d_guide, d_other, d_cost, w, h, dmin, s_begin, s_end, d_keys,
                          d_mean_u8, d_agg, d_workspace, workspace_bytes, nullptr, stream);
}

int smx_dev_aggregate_wta_nbr(const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                              const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                              int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                              size_t workspace_bytes, float* d_nbr, void* stream) {
    SMX_ARG(d_nbr);
    return aggregate_view("smx_dev_aggregate_wta_nbr", p, d_guide, d_other, d_cost, w, h, dmin, s_begin, s_end, d_keys,
                          d_mean_u8, d_agg, d_workspace, workspace_bytes, d_nbr, stream);
}

static int aggregate_pair(const char* who, const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                          const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr, int s_begin,
                          int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                          size_t workspace_bytes, void* stream, float* d_nbr = nullptr, float* d_uq = nullptr) {
    SMX_ARG(p && d_left && d_right && d_keys && d_workspace);
    SMX_ARG(w >= 2 && h >= 1 && s_begin >= 0 && s_end >= s_begin && p->radius >= 0);
    SMX_ARG((d_cost_l != nullptr) == (d_cost_r != nullptr));
    const int64_t n = (int64_t)w * h;
    const int64_t vol = n * (s_end - s_begin);
    const AggCall c = {who, p, 2, {d_left, d_right}, {d_right, d_left}, {d_cost_l, d_cost_r}, {dminl, dminr}, {d_keys, d_keys + n},
                       {d_mean_u8, d_mean_u8 ? d_mean_u8 + n : nullptr}, {d_agg, d_agg ? d_agg + vol : nullptr},
                       {d_nbr, d_nbr ? d_nbr + 3 * n : nullptr}, {d_uq, d_uq ? d_uq + 3 * n : nullptr},
                       w, h, s_begin, s_end, d_workspace, workspace_bytes, (hipStream_t)stream};
    return dev_aggregate(c);
}

int smx_dev_aggregate_wta_pair(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                               int w, int h, int dminl, int dminr, int s_begin, int s_end,
                               int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                               size_t workspace_bytes, void* stream) {
    return aggregate_pair("smx_dev_aggregate_wta_pair", p, d_left, d_right, nullptr, nullptr, w, h, dminl, dminr, s_begin, s_end,
                          d_keys, d_mean_u8, d_agg, d_workspace, workspace_bytes, stream);
}

int smx_dev_aggregate_wta_pair_cost(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                    const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                    int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                    void* d_workspace, size_t workspace_bytes, void* stream) {
    SMX_ARG(d_cost_l && d_cost_r);
    return aggregate_pair("smx_dev_aggregate_wta_pair_cost", p, d_left, d_right, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin,
                          s_end, d_keys, d_mean_u8, d_agg, d_workspace, workspace_bytes, stream);
}

int smx_dev_aggregate_wta_pair_nbr(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                   const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                   int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                   void* d_workspace, size_t workspace_bytes, float* d_nbr, void* stream) {
    SMX_ARG(d_nbr);
    return aggregate_pair("smx_dev_aggregate_wta_pair_nbr", p, d_left, d_right, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin,
                          s_end, d_keys, d_mean_u8, d_agg, d_workspace, workspace_bytes, stream, d_nbr);
}

int smx_dev_aggregate_wta_pair_uq(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                  const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                  int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                  void* d_workspace, size_t workspace_bytes, float* d_nbr, float* d_uq, void* stream) {
    SMX_ARG(d_uq);
    return aggregate_pair("smx_dev_aggregate_wta_pair_uq", p, d_left, d_right, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin,
                          s_end, d_keys, d_mean_u8, d_agg, d_workspace, workspace_bytes, stream, d_nbr, d_uq);
}

int smx_dev_uniqueness(float ratio, const int64_t* d_keys, const float* d_uq, const float* d_disp, float* d_out,
                       float* d_margin, int w, int h, float vmin, float new_val, void* stream) {
    SMX_ARG(uniq_ratio_ok(ratio));
    SMX_ARG(d_keys && d_uq && d_disp && d_out && w >= 1 && h >= 1);
    return launch_uniqueness(ratio, d_keys, d_uq, d_disp, d_out, d_margin, (int64_t)w * h, vmin, new_val, (hipStream_t)stream);
}

int smx_dev_subpixel_pair(int mode, const int64_t* d_keys, const float* d_nbr, const float* d_dmap, const float* d_occlusion,
                          const float* d_filled, int w, int h, int dminl, float* d_sub, float* d_sub_filled, void* stream) {
    SMX_ARG(subpix_mode_ok(mode));
    SMX_ARG(d_keys && d_nbr && d_dmap && d_sub && w >= 1 && h >= 1);
    SMX_ARG(d_sub != d_dmap);
    SMX_ARG(!d_sub_filled || (d_occlusion && d_filled));
    return launch_subpixel_pair(mode, d_keys, d_nbr, d_dmap, d_occlusion, d_filled, w, h, dminl, d_sub, d_sub_filled,
                                (hipStream_t)stream);
}

float smx_subpixel_delta(int mode, float c0, float lo, float hi) {
    return subpix_mode_ok(mode) ? subpixel_delta(mode, c0, lo, hi) : 0.0f;
}

// ---- weighted-median refinement (not in the reference; smx_wmf.hip) ----------------------------------
void smx_default_wmf_params(smx_wmf_params* p) {
    if (!p) return;
    p->radius = 9; p->sigma_s = 9.0; p->sigma_c = 25.5;
}

int smx_wmf_weights(const smx_wmf_params* p, uint16_t* spatial, uint16_t* range) {
    SMX_ARG(wmf_params_ok(p) && spatial && range);
    const double ss = p->sigma_s * p->sigma_s, sc = p->sigma_c * p->sigma_c;
    // (k = 0 / t = 0 directly: a sigma whose square underflows would make 0 / 0 of them)
    for (int k = 0; k <= 2 * p->radius * p->radius; ++k)
        spatial[k] = k == 0 ? 1023 : (uint16_t)floor(1023.0 * exp(-(double)k / ss) + 0.5);
    for (int t = 0; t < 256; ++t)
        range[t] = t == 0 ? 1023 : (uint16_t)floor(1023.0 * exp(-(double)t * t / sc) + 0.5);
    return SMX_OK;
}

int smx_dev_weighted_median(const smx_wmf_params* p, const uint8_t* d_guide, const float* d_disp,
                            const float* d_select, float* d_out, int w, int h, int dmin, int size_d, void* stream) {
    SMX_ARG(wmf_params_ok(p) && d_guide && d_disp && d_out && w >= 1 && h >= 1);
    SMX_ARG(size_d >= 1 && size_d <= 4096 && (long long)dmin + size_d <= INT_MAX);
    SMX_ARG((const void*)d_out != (const void*)d_disp);
    uint16_t ws[2 * 15 * 15 + 1], wc[256];
    smx_wmf_weights(p, ws, wc);
    return launch_weighted_median(p->radius, ws, wc, d_guide, d_disp, d_select, d_out, w, h, dmin, size_d,
                                  (hipStream_t)stream);
}

// ---- speckle removal (not in the reference; smx_speckle.hip) -------------------------------------------
void smx_default_speckle_params(smx_speckle_params* p) {
    if (!p) return;
    p->max_size = 200; p->max_diff = 1.0f;
}

size_t smx_speckle_workspace_bytes(int w, int h) { return shape_ok(w, h, 1, 1) ? speckle_workspace_bytes(w, h) : 0; }

int smx_speckle_geometry(int* tile_cols, int* tile_rows) {
    SMX_ARG(tile_cols && tile_rows);
    speckle_tile(tile_cols, tile_rows);
    return SMX_OK;
}

int smx_dev_speckle_filter(const smx_speckle_params* p, const float* d_disp, float* d_out, int w, int h, float vmin,
                           float new_val, void* d_ws, size_t ws_bytes, void* stream) {
    SMX_ARG(speckle_params_ok(p) && d_disp && d_out && shape_ok(w, h, 1, 1));
    if (!d_ws || ws_bytes < speckle_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_speckle_filter: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    speckle_workspace_bytes(w, h));
    return launch_speckle_filter(p->max_size, p->max_diff, d_disp, d_out, w, h, vmin, new_val, d_ws, (hipStream_t)stream);
}

// ---- census / Hamming matching cost (not in the reference; smx_census.hip) ----------------------------
void smx_default_census_params(smx_census_params* p) {
    if (!p) return;
    p->rx = 4; p->ry = 3; p->th = 62;
}

static int census_nbits(const smx_census_params* p) { return (2 * p->rx + 1) * (2 * p->ry + 1) - 1; }
static int census_t(const smx_census_params* p) { return p->th < census_nbits(p) ? p->th : census_nbits(p); }

int smx_census_bits(const smx_census_params* p) {
    SMX_ARG(census_params_ok(p));
    return census_nbits(p);
}

int smx_dev_census(const smx_census_params* p, const uint8_t* d_img, uint64_t* d_code, int w, int h, int nimages,
                   void* stream) {
    SMX_ARG(census_params_ok(p) && d_img && d_code && w >= 1 && h >= 1 && nimages >= 1);
    return launch_census(p->rx, p->ry, d_img, d_code, w, h, nimages, (hipStream_t)stream);
}

int smx_dev_census_cost_pair(const smx_census_params* p, const uint64_t* d_code, float* d_cost_l, float* d_cost_r, int w,
                             int h, int dminl, int dminr, int s_begin, int s_end, void* stream) {
    SMX_ARG(census_params_ok(p) && d_code && (d_cost_l || d_cost_r));
    SMX_ARG(w >= 1 && h >= 1 && s_begin >= 0 && s_end >= s_begin);
    return launch_census_cost_pair(census_t(p), d_code, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin, s_end,
                                   (hipStream_t)stream);
}

// ---- AD-Census matching cost (not in the reference; smx_adcensus.hip) ----------------------------------
void smx_default_adcensus_params(smx_adcensus_params* p) {
    if (!p) return;
    smx_default_census_params(&p->census);
    p->lambda_census = 30.0; p->lambda_ad = 10.0; p->scale = 127.5; p->colour = 0;
}

int smx_adcensus_tables(const smx_adcensus_params* p, float* tables) {
    SMX_ARG(adcensus_params_ok(p) && tables);
    // (1.0 - exp(-x), not -expm1(-x): the latter is -0.0 at x = 0, which the comb walker's cost check does not admit)
    const double la = (double)(p->colour ? 3 : 1) * p->lambda_ad;
    for (int k = 0; k < 64; ++k) tables[k] = (float)(p->scale * (1.0 - exp(-(double)k / p->lambda_census)));
    for (int s = 0; s <= 765; ++s) tables[64 + s] = (float)(p->scale * (1.0 - exp(-(double)s / la)));
    return SMX_OK;
}

int smx_dev_adcensus_tables(const smx_adcensus_params* p, float* d_tables, void* stream) {
    SMX_ARG(adcensus_params_ok(p) && d_tables);
    float t[SMX_ADCENSUS_TABLE_FLOATS];
    smx_adcensus_tables(p, t);
    SMX_HIP(hipMemcpyAsync(d_tables, t, sizeof(t), hipMemcpyHostToDevice, (hipStream_t)stream));
    SMX_HIP(hipStreamSynchronize((hipStream_t)stream));     // (t lives on this stack)
    return SMX_OK;
}

int smx_dev_adcensus_cost_pair(const smx_adcensus_params* p, const float* d_tables, const uint64_t* d_code,
                               const uint8_t* d_img_l, const uint8_t* d_img_r, int channels, float* d_cost_l, float* d_cost_r,
                               int w, int h, int dminl, int dminr, int s_begin, int s_end, void* stream) {
    SMX_ARG(adcensus_params_ok(p) && d_tables && d_code && d_img_l && d_img_r && (d_cost_l || d_cost_r));
    SMX_ARG(p->colour ? channels == 3 || channels == 4 : channels == 1);
    SMX_ARG(w >= 1 && h >= 1 && s_begin >= 0 && s_end >= s_begin);
    return launch_adcensus_cost_pair(census_t(&p->census), p->colour ? 3 : 1, d_tables, d_code, d_img_l, d_img_r, channels,
                                     d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin, s_end, (hipStream_t)stream);
}

// ---- mutual-information matching cost (not in the reference; smx_mi.hip) --------------------------------
void smx_default_mi_params(smx_mi_params* p) {
    if (!p) return;
    p->iterations = 3; p->init = SMX_MI_INIT_RANDOM; p->seed = 0;
}

int smx_mi_table(const uint32_t* hist, uint8_t* table) {
    SMX_ARG(hist && table);
    mi_table(hist, table);
    return SMX_OK;
}

int smx_dev_mi_table(const uint32_t* hist, uint8_t* d_table, void* stream) {
    SMX_ARG(hist && d_table && ((uintptr_t)d_table & 15) == 0);
    std::vector<uint8_t> t((size_t)SMX_MI_LEVELS * SMX_MI_LEVELS);
    mi_table(hist, t.data());
    SMX_HIP(hipMemcpyAsync(d_table, t.data(), t.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    SMX_HIP(hipStreamSynchronize((hipStream_t)stream));     // (t lives in this call)
    return SMX_OK;
}

int smx_dev_mi_histogram(const uint8_t* d_img_l, const uint8_t* d_img_r, const float* d_map, float occlusion_mark,
                         uint32_t* d_hist, int w, int h, void* stream) {
    SMX_ARG(d_img_l && d_img_r && d_map && d_hist);
    if (!shape_ok(w, h, 1, 1)) return fail(SMX_E_ARG, "smx_dev_mi_histogram: %s", PLANE_SHAPES);
    return launch_mi_histogram(d_img_l, d_img_r, d_map, occlusion_mark, d_hist, w, h, (hipStream_t)stream);
}

int smx_dev_mi_random_map(float* d_map, int w, int h, int dmin, int size_d, uint32_t seed, void* stream) {
    SMX_ARG(d_map != nullptr);
    if (!shape_ok(w, h, size_d, INT_MAX)) return fail(SMX_E_ARG, "smx_dev_mi_random_map: %s and size_d >= 1", PLANE_SHAPES);
    return launch_mi_random_map(d_map, w, h, dmin, size_d, seed, (hipStream_t)stream);
}

int smx_dev_mi_cost_pair(const uint8_t* d_table, const uint8_t* d_img_l, const uint8_t* d_img_r, float* d_cost_l,
                         float* d_cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end, void* stream) {
    SMX_ARG(d_table && ((uintptr_t)d_table & 15) == 0 && d_img_l && d_img_r && (d_cost_l || d_cost_r));
    SMX_ARG(w >= 1 && h >= 1 && s_begin >= 0 && s_end >= s_begin);
    return launch_mi_cost_pair(d_table, d_img_l, d_img_r, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin, s_end,
                               (hipStream_t)stream);
}

// ---- ZNCC window matching cost (not in the reference; smx_zncc.hip) -------------------------------------
void smx_default_zncc_params(smx_zncc_params* p) {
    if (!p) return;
    p->rx = 3; p->ry = 3;
}

int smx_zncc_window(const smx_zncc_params* p) {
    SMX_ARG(zncc_params_ok(p));
    return (2 * p->rx + 1) * (2 * p->ry + 1);
}

int smx_zncc_geometry(int* cols, int* rows) {
    SMX_ARG(cols && rows);
    zncc_geometry(cols, rows);
    return SMX_OK;
}

int smx_dev_zncc_moments(const smx_zncc_params* p, const uint8_t* d_img, uint64_t* d_mom, int w, int h, int nimages, void* stream) {
    if (!zncc_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_zncc_moments: %s", ZNCC_RANGES);
    SMX_ARG(d_img && d_mom && ((uintptr_t)d_mom & 7) == 0 && w >= 1 && h >= 1 && nimages >= 1);
    return launch_zncc_moments(p->rx, p->ry, d_img, d_mom, w, h, nimages, (hipStream_t)stream);
}

int smx_dev_zncc_cost_pair(const smx_zncc_params* p, const uint64_t* d_mom, const uint8_t* d_img_l, const uint8_t* d_img_r,
                           float* d_cost_l, float* d_cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end,
                           void* stream) {
    if (!zncc_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_zncc_cost_pair: %s", ZNCC_RANGES);
    SMX_ARG(d_mom && ((uintptr_t)d_mom & 7) == 0 && d_img_l && d_img_r && (d_cost_l || d_cost_r));
    SMX_ARG(w >= 1 && h >= 1 && s_begin >= 0 && s_end >= s_begin);
    return launch_zncc_cost_pair(p->rx, p->ry, d_mom, d_img_l, d_img_r, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin, s_end,
                                 (hipStream_t)stream);
}

// ---- semi-global matching (not in the reference; smx_sgm.hip) -----------------------------------------
void smx_default_sgm_params(smx_sgm_params* p) {
    if (!p) return;
    p->p1 = 10; p->p2 = 120; p->paths = 8;
}

size_t smx_sgm_workspace_bytes(int w, int h, int size_d, int nviews) {
    return shape_ok(w, h, size_d, SMX_SGM_MAX_D) && (nviews == 1 || nviews == 2) ? sgm_workspace_bytes(w, h, size_d, nviews) : 0;
}

static int sgm_wta_pair(const char* who, const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h,
                        int size_d, int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes,
                        void* stream) {
    if (!sgm_params_ok(p))
        return fail(SMX_E_ARG, "%s: %s", who, SGM_RANGES);
    if (!shape_ok(w, h, size_d, SMX_SGM_MAX_D))
        return fail(SMX_E_ARG, "%s: %s", who, SGM_SHAPES);
    SMX_ARG((d_cost_l || d_cost_r) && d_keys);
    const size_t need = sgm_workspace_bytes(w, h, size_d, d_cost_l && d_cost_r ? 2 : 1);
    if (!d_ws || ws_bytes < need)
        return fail(SMX_E_WS, "%s: workspace of %zu bytes, %zu needed", who, d_ws ? ws_bytes : (size_t)0, need);
    return launch_sgm_wta_pair(p->p1, p->p2, p->paths, d_cost_l, d_cost_r, w, h, size_d, d_keys, d_agg, d_nbr, d_uq, d_ws,
                               (hipStream_t)stream);
}

int smx_dev_sgm_wta_pair(const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                         int64_t* d_keys, float* d_agg, float* d_nbr, void* d_ws, size_t ws_bytes, void* stream) {
    return sgm_wta_pair("smx_dev_sgm_wta_pair", p, d_cost_l, d_cost_r, w, h, size_d, d_keys, d_agg, d_nbr, nullptr, d_ws, ws_bytes,
                        stream);
}

int smx_dev_sgm_wta_pair_uq(const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                            int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes,
                            void* stream) {
    SMX_ARG(d_uq);
    return sgm_wta_pair("smx_dev_sgm_wta_pair_uq", p, d_cost_l, d_cost_r, w, h, size_d, d_keys, d_agg, d_nbr, d_uq, d_ws, ws_bytes,
                        stream);
}

// ---- hierarchical belief propagation (not in the reference; smx_bp.hip) ---------------------------------------------
void smx_default_bp_params(smx_bp_params* p) {
    if (!p) return;
    p->step = 20; p->trunc = 60; p->iterations = 5; p->levels = 4; p->data_scale = 1.0f;
}

size_t smx_bp_workspace_bytes(int w, int h, int size_d, int levels, int nviews) {
    return shape_ok(w, h, size_d, SMX_BP_MAX_D) && levels >= 1 && levels <= 8 && (nviews == 1 || nviews == 2)
               ? bp_workspace_bytes(w, h, size_d, levels, nviews) : 0;
}

int smx_dev_bp_wta_pair(const smx_bp_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                        int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    if (!bp_params_ok(p))
        return fail(SMX_E_ARG, "smx_dev_bp_wta_pair: %s", BP_RANGES);
    if (!shape_ok(w, h, size_d, SMX_BP_MAX_D)) return fail(SMX_E_ARG, "smx_dev_bp_wta_pair: %s", BP_SHAPES);
    SMX_ARG((d_cost_l || d_cost_r) && d_keys);
    const size_t need = bp_workspace_bytes(w, h, size_d, p->levels, d_cost_l && d_cost_r ? 2 : 1);
    if (!d_ws || ws_bytes < need)
        return fail(SMX_E_WS, "smx_dev_bp_wta_pair: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
    return launch_bp_wta_pair(p, d_cost_l, d_cost_r, w, h, size_d, d_keys, d_agg, d_nbr, d_uq, d_ws, (hipStream_t)stream);
}

// ---- scan-line optimisation with colour-adaptive penalties (not in the reference; smx_scanline.hip) -----------------
void smx_default_scanline_params(smx_scanline_params* p) {
    if (!p) return;
    p->p1 = 127; p->p2 = 382; p->tau_so = 15; p->paths = 4;
}

size_t smx_scanline_workspace_bytes(int w, int h, int size_d, int nviews) {
    return shape_ok(w, h, size_d, SMX_SGM_MAX_D) && (nviews == 1 || nviews == 2) ? scanline_workspace_bytes(w, h, size_d, nviews) : 0;
}

int smx_dev_scanline_wta_pair(const smx_scanline_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels,
                              const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d, int dminl, int dminr,
                              int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    if (!scanline_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_scanline_wta_pair: %s", SCANLINE_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, SMX_SGM_MAX_D)) return fail(SMX_E_ARG, "smx_dev_scanline_wta_pair: %s", SGM_SHAPES);
    SMX_ARG(d_guide_l && d_guide_r && (d_cost_l || d_cost_r) && d_keys);
    const size_t need = scanline_workspace_bytes(w, h, size_d, d_cost_l && d_cost_r ? 2 : 1);
    if (!d_ws || ws_bytes < need)
        return fail(SMX_E_WS, "smx_dev_scanline_wta_pair: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
    return launch_scanline_wta_pair(p, d_guide_l, d_guide_r, channels, d_cost_l, d_cost_r, w, h, size_d, dminl, dminr, d_keys,
                                    d_agg, d_nbr, d_uq, d_ws, (hipStream_t)stream);
}

// ---- colour-guided filter aggregation (not in the reference; smx_cgf.hip) -----------------------------------------
static bool cgf_shape_ok(int w, int h) { return shape_ok(w, h, 1, 1) && h <= CGF_MAX_H; }

size_t smx_cgf_workspace_bytes(int w, int h, int nslices, int nviews) {
    return cgf_shape_ok(w, h) && nslices >= 1 && (nviews == 1 || nviews == 2) ? cgf_workspace_bytes(w, h, nslices, nviews) : 0;
}

int smx_dev_cgf_wta_pair(const smx_params* p, const uint8_t* d_rgb_l, const uint8_t* d_rgb_r, int channels,
                         const float* d_cost_l, const float* d_cost_r, int w, int h, int s_begin, int s_end, int64_t* d_keys,
                         float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    SMX_ARG(p && p->radius >= 0 && (channels == 3 || channels == 4));
    if (!cgf_shape_ok(w, h)) return fail(SMX_E_ARG, "smx_dev_cgf_wta_pair: %s", CGF_SHAPES);
    SMX_ARG(s_begin >= 0 && s_end > s_begin && d_keys);
    SMX_ARG((d_cost_l || d_cost_r) && !d_rgb_l == !d_cost_l && !d_rgb_r == !d_cost_r);
    const int nviews = d_cost_l && d_cost_r ? 2 : 1;
    const int chunk = d_ws ? cgf_chunk(w, h, nviews, ws_bytes, s_end - s_begin, g_max_chunk) : 0;
    if (chunk < 1)
        return fail(SMX_E_WS, "smx_dev_cgf_wta_pair: workspace of %zu bytes, %zu needed for one slice in flight",
                    d_ws ? ws_bytes : (size_t)0, cgf_workspace_bytes(w, h, 1, nviews));
    return launch_cgf_wta_pair(p, d_rgb_l, d_rgb_r, channels, d_cost_l, d_cost_r, w, h, s_begin, s_end, d_keys, d_agg, d_nbr,
                               d_uq, d_ws, chunk, (hipStream_t)stream);
}

// ---- cross-based aggregation (not in the reference; smx_cross.hip) ---------------------------------------------------
void smx_default_cross_params(smx_cross_params* p) {
    if (!p) return;
    p->l1 = 34; p->l2 = 17; p->tau1 = 20; p->tau2 = 6; p->iterations = 4;
}

size_t smx_cross_workspace_bytes(int w, int h, int nslices, int nviews) {
    return shape_ok(w, h, 1, 1) && nslices >= 1 && (nviews == 1 || nviews == 2) ? cross_workspace_bytes(w, h, nslices, nviews) : 0;
}

int smx_dev_cross_arms(const smx_cross_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels, int w, int h,
                       uint32_t* d_arms, void* stream) {
    if (!cross_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_cross_arms: %s", CROSS_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, 1, 1)) return fail(SMX_E_ARG, "smx_dev_cross_arms: %s", PLANE_SHAPES);
    SMX_ARG((d_guide_l || d_guide_r) && d_arms);
    return launch_cross_arms(p, d_guide_l, d_guide_r, channels, w, h, d_arms, (hipStream_t)stream);
}

int smx_dev_cross_wta_pair(const smx_cross_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels,
                           const float* d_cost_l, const float* d_cost_r, int w, int h, int s_begin, int s_end, int64_t* d_keys,
                           float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    if (!cross_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_cross_wta_pair: %s", CROSS_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, 1, 1)) return fail(SMX_E_ARG, "smx_dev_cross_wta_pair: %s", PLANE_SHAPES);
    SMX_ARG(s_begin >= 0 && s_end > s_begin && d_keys);
    SMX_ARG((d_cost_l || d_cost_r) && !d_guide_l == !d_cost_l && !d_guide_r == !d_cost_r);
    const int nviews = d_cost_l && d_cost_r ? 2 : 1;
    const int chunk = d_ws ? cross_chunk(w, h, nviews, ws_bytes, s_end - s_begin, g_max_chunk) : 0;
    if (chunk < 1)
        return fail(SMX_E_WS, "smx_dev_cross_wta_pair: workspace of %zu bytes, %zu needed for one slice in flight",
                    d_ws ? ws_bytes : (size_t)0, cross_workspace_bytes(w, h, 1, nviews));
    return launch_cross_wta_pair(p, d_guide_l, d_guide_r, channels, d_cost_l, d_cost_r, w, h, s_begin, s_end, d_keys, d_agg,
                                 d_nbr, d_uq, d_ws, chunk, (hipStream_t)stream);
}

// ---- region voting on the cross arms (not in the reference; smx_vote.hip) -------------------------------------------
void smx_default_vote_params(smx_vote_params* p) {
    if (!p) return;
    p->tau_s = 20; p->tau_h_pct = 40; p->iterations = 5; p->interpolate = 1;
}

size_t smx_vote_workspace_bytes(int w, int h) { return shape_ok(w, h, 1, VOTE_MAX_D) ? vote_workspace_bytes(w, h) : 0; }

int smx_vote_geometry(int* tile_cols, int* tile_rows) {
    SMX_ARG(tile_cols && tile_rows);
    vote_tile(tile_cols, tile_rows);
    return SMX_OK;
}

int smx_dev_region_vote(const smx_vote_params* p, const uint32_t* d_arms, const uint8_t* d_guide, int channels, const float* d_disp,
                        const float* d_disp_r, float* d_out, int w, int h, int dmin, int size_d, int d_lr, void* d_ws,
                        size_t ws_bytes, void* stream) {
    if (!vote_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_region_vote: %s", VOTE_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, VOTE_MAX_D)) return fail(SMX_E_ARG, "smx_dev_region_vote: %s", VOTE_SHAPES);
    SMX_ARG(d_arms && d_disp && d_out);
    SMX_ARG(d_guide || !p->interpolate || !d_disp_r);
    if (!d_ws || ws_bytes < vote_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_region_vote: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    vote_workspace_bytes(w, h));
    return launch_region_vote(p, d_arms, d_guide, channels, d_disp, d_disp_r, d_out, w, h, dmin, size_d, d_lr, d_ws,
                              (hipStream_t)stream);
}

// ---- depth-discontinuity adjustment from the aggregated costs (not in the reference; smx_adjust.hip) -------------------
void smx_default_adjust_params(smx_adjust_params* p) {
    if (!p) return;
    p->tau_e = 2; p->vertical = 1; p->iterations = 1;
}

size_t smx_adjust_workspace_bytes(int w, int h) { return shape_ok(w, h, 1, ADJ_MAX_D) ? adjust_workspace_bytes(w, h) : 0; }

int smx_adjust_geometry(int* cols, int* rows) {
    SMX_ARG(cols && rows);
    adjust_tile(cols, rows);
    return SMX_OK;
}

int smx_dev_discontinuity_adjust(const smx_adjust_params* p, const float* d_disp, const float* d_agg, float* d_out, int w, int h,
                                 int dmin, int size_d, int subpix_mode, float* d_sub, void* d_ws, size_t ws_bytes, void* stream) {
    if (!adjust_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_discontinuity_adjust: %s", ADJUST_RANGES);
    if (!shape_ok(w, h, size_d, ADJ_MAX_D)) return fail(SMX_E_ARG, "smx_dev_discontinuity_adjust: %s", ADJUST_SHAPES);
    SMX_ARG(d_disp && d_agg && d_out);
    if (d_sub ? !subpix_mode_ok(subpix_mode) : subpix_mode != 0 && !subpix_mode_ok(subpix_mode))
        return fail(SMX_E_ARG, "smx_dev_discontinuity_adjust: subpix_mode must be SMX_SUBPIX_PARABOLA or SMX_SUBPIX_EQUIANGULAR "
                               "(or 0 without d_sub)");
    if (!d_ws || ws_bytes < adjust_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_discontinuity_adjust: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    adjust_workspace_bytes(w, h));
    return launch_discontinuity_adjust(p, d_disp, d_agg, d_out, w, h, dmin, size_d, subpix_mode, d_sub, d_ws, (hipStream_t)stream);
}

// ---- cross-scale cost aggregation (not in the reference; smx_cscale.hip) -----------------------------------------------
void smx_default_cscale_params(smx_cscale_params* p) {
    if (!p) return;
    p->scales = 4; p->lambda = 1.0;
}

int smx_cscale_weights(const smx_cscale_params* p, float* wt) {
    if (!cscale_params_ok(p)) return fail(SMX_E_ARG, "smx_cscale_weights: %s", CSCALE_RANGES);
    SMX_ARG(wt != nullptr);
    cscale_weights(p, wt);
    return SMX_OK;
}

int smx_cscale_level(int w, int h, int dmin, int size_d, int s, int* w_s, int* h_s, int* dmin_s, int* size_d_s) {
    SMX_ARG(w >= 1 && h >= 1 && size_d >= 1 && s >= 0 && s <= 30 && w_s && h_s && dmin_s && size_d_s);
    cscale_level(w, h, dmin, size_d, s, w_s, h_s, dmin_s, size_d_s);
    return SMX_OK;
}

int smx_pyr_down_geometry(int* cols, int* rows) {
    SMX_ARG(cols && rows);
    pyr_down_tile(cols, rows);
    return SMX_OK;
}

int smx_dev_pyr_down(const uint8_t* d_src, uint8_t* d_dst, int w, int h, int channels, void* stream) {
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, 1, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_dev_pyr_down: %s", PLANE_SHAPES);
    SMX_ARG(d_src && d_dst);
    return launch_pyr_down(d_src, d_dst, w, h, channels, (hipStream_t)stream);
}

int smx_dev_cscale_wta_pair(const smx_cscale_params* p, const float* const* d_agg_l, const float* const* d_agg_r, int w, int h,
                            int dminl, int dminr, int size_d, int64_t* d_keys, float* d_out, float* d_nbr, float* d_uq,
                            void* stream) {
    if (!cscale_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_cscale_wta_pair: %s", CSCALE_RANGES);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_dev_cscale_wta_pair: %s", CSCALE_SHAPES);
    SMX_ARG((d_agg_l || d_agg_r) && d_keys);
    const float* const* views[2] = {d_agg_l, d_agg_r};
    const int dmins[2] = {dminl, dminr};
    for (int v = 0; v < 2; ++v) {
        if (!views[v]) continue;
        // (the label range of every level must exist as ints)
        if (dmins[v] < -(1 << 29) || dmins[v] > (1 << 29))
            return fail(SMX_E_ARG, "smx_dev_cscale_wta_pair: the labels of view %d start at %d, outside +-2^29", v, dmins[v]);
        for (int s = 0; s < p->scales; ++s)
            if (!views[v][s] || ((uintptr_t)views[v][s] & 3) != 0)
                return fail(SMX_E_ARG, "smx_dev_cscale_wta_pair: the level-%d volume of view %d is NULL or not 4-byte aligned", s, v);
    }
    return launch_cscale_wta_pair(p, d_agg_l, d_agg_r, w, h, dminl, dminr, size_d, d_keys, d_out, d_nbr, d_uq, (hipStream_t)stream);
}

// ---- PatchMatch stereo (not in the reference; smx_patchmatch.hip) --------------------------------------------------------
void smx_default_pm_params(smx_pm_params* p) {
    if (!p) return;
    p->radius = 8; p->gamma = 10.0; p->iterations = 4; p->max_slope = 2.0; p->seed = 0;
}

int smx_pm_weights(const smx_pm_params* p, float* tab) {
    if (!pm_params_ok(p)) return fail(SMX_E_ARG, "smx_pm_weights: %s", PM_RANGES);
    SMX_ARG(tab != nullptr);
    pm_weights(p, tab);
    return SMX_OK;
}

uint32_t smx_pm_hash(uint32_t seed, uint32_t view, uint32_t pixel, uint32_t draw) { return pm_hash_host(seed, view, pixel, draw); }

size_t smx_pm_workspace_bytes(int w, int h) { return pm_shape_ok(w, h, 1, 0, 0) ? pm_workspace_bytes(w, h) : 0; }

int smx_pm_geometry(int* cols, int* rows) {
    SMX_ARG(cols && rows);
    pm_tile(cols, rows);
    return SMX_OK;
}

int smx_dev_patchmatch_pair(const smx_params* p, const smx_pm_params* pm, const uint8_t* d_left, const uint8_t* d_right, int w,
                            int h, int size_d, int dminl, int dminr, float* d_planes, float* d_cost, float* d_disp,
                            float* d_label, void* d_ws, size_t ws_bytes, void* stream) {
    if (!pm_params_ok(pm)) return fail(SMX_E_ARG, "smx_dev_patchmatch_pair: %s", PM_RANGES);
    if (!pm_shape_ok(w, h, size_d, dminl, dminr)) return fail(SMX_E_ARG, "smx_dev_patchmatch_pair: %s", PM_SHAPES);
    SMX_ARG(p && d_left && d_right && d_planes && d_cost && d_disp && d_label);
    if (!d_ws || ws_bytes < pm_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_patchmatch_pair: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    pm_workspace_bytes(w, h));
    return launch_patchmatch_pair(p, pm, d_left, d_right, w, h, size_d, dminl, dminr, d_planes, d_cost, d_disp, d_label, d_ws,
                                  (hipStream_t)stream);
}

int smx_dev_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* d_left, const uint8_t* d_right, int w, int h,
                          int size_d, int dminl, int dminr, const float* d_planes, float* d_cost, void* d_ws, size_t ws_bytes,
                          void* stream) {
    if (!pm_params_ok(pm)) return fail(SMX_E_ARG, "smx_dev_pm_plane_cost: %s", PM_RANGES);
    if (!pm_shape_ok(w, h, size_d, dminl, dminr)) return fail(SMX_E_ARG, "smx_dev_pm_plane_cost: %s", PM_SHAPES);
    SMX_ARG(p && d_left && d_right && d_planes && d_cost);
    if (!d_ws || ws_bytes < pm_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_pm_plane_cost: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    pm_workspace_bytes(w, h));
    return launch_pm_plane_cost(p, pm, d_left, d_right, w, h, size_d, dminl, dminr, d_planes, d_cost, d_ws, (hipStream_t)stream);
}

int smx_dev_pm_sub_filled(const float* d_disp, const float* d_kept, const float* d_filled, int w, int h, int dminl, float* d_out,
                          void* stream) {
    if (!pm_shape_ok(w, h, 1, dminl, 0)) return fail(SMX_E_ARG, "smx_dev_pm_sub_filled: %s", PM_SHAPES);
    SMX_ARG(d_disp && d_kept && d_filled && d_out);
    return launch_pm_sub_filled(d_disp, d_kept, d_filled, (size_t)w * h, dminl, d_out, (hipStream_t)stream);
}

// ---- the permeability filter (not in the reference; smx_perm.hip) ---------------------------------------------------------
void smx_default_perm_params(smx_perm_params* p) {
    if (!p) return;
    p->sigma = 32.0;
}

int smx_perm_table(const smx_perm_params* p, float* t) {
    if (!perm_params_ok(p)) return fail(SMX_E_ARG, "smx_perm_table: %s", PERM_RANGES);
    SMX_ARG(t != nullptr);
    perm_table(p, t);
    return SMX_OK;
}

size_t smx_perm_workspace_bytes(int w, int h, int size_d, int nviews) {
    return shape_ok(w, h, size_d, WIDE_MAX_D) && (nviews == 1 || nviews == 2) ? perm_workspace_bytes(w, h, size_d, nviews) : 0;
}

int smx_dev_permeability_wta_pair(const smx_perm_params* p, const float* d_vol_l, const float* d_vol_r, const uint8_t* d_guide_l,
                                  const uint8_t* d_guide_r, int channels, int w, int h, int dminl, int dminr, int size_d,
                                  int64_t* d_keys, float* d_out, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    if (!perm_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_permeability_wta_pair: %s", PERM_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_dev_permeability_wta_pair: %s", PERM_SHAPES);
    SMX_ARG((d_vol_l || d_vol_r) && !d_guide_l == !d_vol_l && !d_guide_r == !d_vol_r);
    SMX_ARG(d_keys || (!d_nbr && !d_uq));
    SMX_ARG(dminl >= -(1 << 29) && dminl <= (1 << 29) && dminr >= -(1 << 29) && dminr <= (1 << 29));
    if ((((uintptr_t)d_vol_l | (uintptr_t)d_vol_r | (uintptr_t)d_out | (uintptr_t)d_ws) & 3) != 0)
        return fail(SMX_E_ARG, "smx_dev_permeability_wta_pair: a volume or the workspace is not 4-byte aligned");
    const int nviews = d_vol_l && d_vol_r ? 2 : 1;
    const int chunk = d_ws ? perm_chunk(w, h, nviews, ws_bytes, size_d, d_out == nullptr, g_max_chunk) : 0;
    if (chunk < 1)
        return fail(SMX_E_WS, "smx_dev_permeability_wta_pair: workspace of %zu bytes, %zu needed for one slice in flight",
                    d_ws ? ws_bytes : (size_t)0, (size_t)nviews * w * h * sizeof(float) * (d_out ? 3 : 4));
    float table[256];
    perm_table(p, table);
    return launch_perm_wta_pair(table, d_vol_l, d_vol_r, d_guide_l, d_guide_r, channels, w, h, size_d, d_keys, d_out, d_nbr, d_uq,
                                d_ws, chunk, (hipStream_t)stream);
}

// ---- the non-local tree filter (not in the reference; smx_tree.hip, smx_tree_host.h) --------------------------------------
void smx_default_tree_params(smx_tree_params* p) {
    if (!p) return;
    p->sigma = 25.5;
}

static bool tree_shape_ok(int w, int h) { return w >= 1 && h >= 1 && (long long)w * h < (1ll << 31); }

size_t smx_tree_bytes(int w, int h) { return tree_shape_ok(w, h) ? tree_layout((size_t)w * h).bytes : 0; }

int smx_tree_build(const uint8_t* guide, int channels, int w, int h, void* blob) {
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!tree_shape_ok(w, h)) return fail(SMX_E_ARG, "smx_tree_build: %s", PLANE_SHAPES);
    SMX_ARG(guide && blob);
    if (((uintptr_t)blob & 3) != 0) return fail(SMX_E_ARG, "smx_tree_build: the blob is not 4-byte aligned");
    try {
        tree_build(guide, channels, w, h, (uint8_t*)blob);
    } catch (const std::bad_alloc&) {
        return fail(SMX_E_HIP, "smx_tree_build: out of host memory");
    }
    return SMX_OK;
}

int smx_tree_tables(const smx_tree_params* p, float* t, float* u) {
    if (!tree_params_ok(p)) return fail(SMX_E_ARG, "smx_tree_tables: %s", TREE_RANGES);
    SMX_ARG(t != nullptr && u != nullptr);
    tree_tables(p, t, u);
    return SMX_OK;
}

size_t smx_tree_workspace_bytes(int w, int h, int size_d, int nviews) {
    return shape_ok(w, h, size_d, WIDE_MAX_D) && (nviews == 1 || nviews == 2) ? tree_workspace_bytes(w, h, size_d, nviews) : 0;
}

int smx_dev_tree_wta_pair(const smx_tree_params* p, const float* d_vol_l, const float* d_vol_r, const void* d_tree_l,
                          const void* d_tree_r, int w, int h, int dminl, int dminr, int size_d, int64_t* d_keys, float* d_out,
                          float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream) {
    if (!tree_params_ok(p)) return fail(SMX_E_ARG, "smx_dev_tree_wta_pair: %s", TREE_RANGES);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_dev_tree_wta_pair: %s", PERM_SHAPES);
    SMX_ARG((d_vol_l || d_vol_r) && !d_tree_l == !d_vol_l && !d_tree_r == !d_vol_r);
    SMX_ARG(d_keys || (!d_nbr && !d_uq));
    SMX_ARG(dminl >= -(1 << 29) && dminl <= (1 << 29) && dminr >= -(1 << 29) && dminr <= (1 << 29));
    if ((((uintptr_t)d_vol_l | (uintptr_t)d_vol_r | (uintptr_t)d_out | (uintptr_t)d_ws | (uintptr_t)d_tree_l | (uintptr_t)d_tree_r) & 3) != 0)
        return fail(SMX_E_ARG, "smx_dev_tree_wta_pair: a volume, a tree or the workspace is not 4-byte aligned");
    const int nviews = d_vol_l && d_vol_r ? 2 : 1;
    const int chunk = d_ws ? tree_chunk(w, h, nviews, ws_bytes, size_d, d_out == nullptr, g_max_chunk) : 0;
    if (chunk < 1)
        return fail(SMX_E_WS, "smx_dev_tree_wta_pair: workspace of %zu bytes, %zu needed for one slice in flight",
                    d_ws ? ws_bytes : (size_t)0, (size_t)nviews * w * h * sizeof(float) * (d_out ? 1 : 2));
    float t[256], u[256];
    tree_tables(p, t, u);
    return launch_tree_wta_pair(t, u, d_vol_l, d_vol_r, (const uint8_t*)d_tree_l, (const uint8_t*)d_tree_r, w, h, size_d, d_keys,
                                d_out, d_nbr, d_uq, d_ws, chunk, (hipStream_t)stream);
}

// Test hook (not in include/smx.h): the natural-order winner-take-all pass of the aggregations (wta_launch, smx_wta.h) over one
// materialised volume d_q [count][h][w], fresh keys out -- what tests/test_gpu_cscale.py holds the one-scale combination to.
__attribute__((visibility("default"))) int smx_debug_wta_natural(const float* d_q, int w, int h, int count, int64_t* d_keys,
                                                                 void* stream) {
    SMX_ARG(d_q && d_keys && count >= 1);
    if (!shape_ok(w, h, count, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_debug_wta_natural: %s", CSCALE_SHAPES);
    return wta_launch(WTA_NATURAL, 1, &d_q, &d_keys, nullptr, nullptr, w, h, (size_t)w * h, count, 0, nullptr, 0, true,
                      (hipStream_t)stream);
}

int smx_dev_filter(const smx_params* p, const uint8_t* d_image, int w, int h, uint8_t* d_mean,
                   float* d_var, void* stream) {
    SMX_ARG(p && d_image && d_mean && d_var && w >= 1 && h >= 1 && p->radius >= 0);
    return launch_filter(p, d_image, d_mean, d_var, w, h, (hipStream_t)stream);
}

}  // extern "C"
