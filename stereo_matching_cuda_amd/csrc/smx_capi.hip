// smx_capi.hip -- the C-ABI of include/smx.h: argument checks, the calling thread's knobs, stage timing, the host-pointer
// wrappers that mirror the reference's per-stage functions, and the persistent context.  Every aggregation goes through
// run_aggregation into smx_agg.hip.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "smx_agg.h"
#include "smx_agg_v4.h"
#include "smx_agg_v5.h"
#include "smx_launch.h"

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

// Every aggregation of this file -- the device entries with forced = the thread's path, the context with its own -- meets the
// thread's knobs here and nowhere else.  A context call, too, takes keys_fresh and max_chunk from the CALLING thread, and
// smx_last_agg_chunk keeps describing the thread's last fused aggregation (smx.h), so a multi-kernel call leaves it alone.
static int run_aggregation(const AggCall& c, int forced) {
    AggOpts opt;
    opt.keys_fresh = g_keys_fresh != 0;
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

// RAII device allocation for the host-pointer wrappers.
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T> T* as() { return (T*)p; }
};

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

const char* smx_version(void) { return "smx-hip gfx950 0.11 (sub-pixel disparity from the winner's neighbouring costs: smx_dev_subpixel_pair; weighted-median refinement of the filled map: smx_weighted_median; comb walker: items pipelined across tickets, q scratch in row pairs, cost volumes on the comb walker; WTA winner in the float domain; guidance in three launches; two 512-thread workgroups per CU)"; }

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
    if (rc) return rc;
    if (st != 0)
        return fail(SMX_E_HIP, "fused aggregation: hand-off wait of work item %u timed out (results invalid)",
                    st - 1);
    return SMX_OK;
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
    return run_aggregation(c, g_agg_path);
}

// smx_dev_aggregate_wta and, with d_nbr != NULL (the view's state planes, smx_common.h nbr_merge), its _nbr form
static int aggregate_view(const char* who, const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                          const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                          int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                          size_t workspace_bytes, float* d_nbr, void* stream) {
    SMX_ARG(p && d_guide && d_keys && d_workspace);
    SMX_ARG(d_cost || d_other);
    SMX_ARG(w >= 2 && h >= 1 && s_begin >= 0 && s_end >= s_begin && p->radius >= 0);
    const AggCall c = {who, p, 1, {d_guide}, {d_other}, {d_cost}, {dmin}, {d_keys}, {d_mean_u8}, {d_agg}, {d_nbr},
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
                          size_t workspace_bytes, void* stream, float* d_nbr = nullptr) {
    SMX_ARG(p && d_left && d_right && d_keys && d_workspace);
    SMX_ARG(w >= 2 && h >= 1 && s_begin >= 0 && s_end >= s_begin && p->radius >= 0);
    SMX_ARG((d_cost_l != nullptr) == (d_cost_r != nullptr));
    const int64_t n = (int64_t)w * h;
    const int64_t vol = n * (s_end - s_begin);
    const AggCall c = {who, p, 2, {d_left, d_right}, {d_right, d_left}, {d_cost_l, d_cost_r}, {dminl, dminr}, {d_keys, d_keys + n},
                       {d_mean_u8, d_mean_u8 ? d_mean_u8 + n : nullptr}, {d_agg, d_agg ? d_agg + vol : nullptr},
                       {d_nbr, d_nbr ? d_nbr + 3 * n : nullptr},
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

static bool subpix_mode_ok(int mode) { return mode == SMX_SUBPIX_PARABOLA || mode == SMX_SUBPIX_EQUIANGULAR; }

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

/* ------------------------------------------------------------------------------------------
 * host-pointer stage API (reference L2 wrappers: allocate, upload, run, download, free)
 * ---------------------------------------------------------------------------------------- */

int smx_rgb_to_grayscale(const smx_params* p, const uint8_t* h_rgb, int64_t n, int channels,
                         uint8_t* h_gray) {
    SMX_ARG(p && h_rgb && h_gray && n > 0 && channels >= 3);
    DevBuf rgb, gray;
    SMX_HIP(rgb.alloc((size_t)n * channels));
    SMX_HIP(gray.alloc((size_t)n));
    SMX_HIP(hipMemcpy(rgb.p, h_rgb, (size_t)n * channels, hipMemcpyHostToDevice));
    int rc = smx_dev_rgb_to_grayscale(p, rgb.as<uint8_t>(), n, channels, gray.as<uint8_t>(), nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(h_gray, gray.p, (size_t)n, hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_compute_cost(const smx_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w1,
                     int w2, int h1, int h2, int size_d, int dmin) {
    SMX_ARG(p && i1 && i2 && cost && size_d >= 1);
    SMX_ARG(w1 >= 2 && w1 == w2 && h1 >= 1 && h1 == h2);
    const size_t n = (size_t)w1 * h1;
    DevBuf d1, d2, dc;
    SMX_HIP(d1.alloc(n));
    SMX_HIP(d2.alloc(n));
    SMX_HIP(dc.alloc(n * size_d * sizeof(float)));
    SMX_HIP(hipMemcpy(d1.p, i1, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(d2.p, i2, n, hipMemcpyHostToDevice));
    int rc = smx_dev_cost_volume(p, d1.as<uint8_t>(), d2.as<uint8_t>(), dc.as<float>(), w1, w2, h1,
                                 dmin, 0, size_d, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(cost, dc.p, n * size_d * sizeof(float), hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_integral(const float* image, float* integral, int width, int height) {
    SMX_ARG(image && integral && width >= 1 && height >= 1);
    const size_t bytes = (size_t)width * height * sizeof(float);
    DevBuf d;
    SMX_HIP(d.alloc(bytes));
    SMX_HIP(hipMemcpy(d.p, image, bytes, hipMemcpyHostToDevice));
    int rc = smx_dev_integral(d.as<float>(), d.as<float>(), width, height, 1, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(integral, d.p, bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}

static size_t pick_ws_bytes(int w, int h, int size_d) {
    // keep at most ~2 GiB of slices in flight for the host-pointer wrappers
    const size_t one = smx_agg_workspace_bytes(w, h, 1);
    const size_t all = smx_agg_workspace_bytes(w, h, size_d);
    const size_t cap = (size_t)2 << 30;
    if (all <= cap) return all;
    return one > cap ? one : cap;
}

int smx_compute_guided_filter(const smx_params* p, const uint8_t* i, const float* cost,
                              float* filter_cost, float* disp_map, uint8_t* mean, float* agg, int w,
                              int h, int size_d, int dmin) {
    SMX_ARG(p && i && cost && filter_cost && disp_map && size_d >= 1 && w >= 2 && h >= 1);
    const size_t n = (size_t)w * h;
    const size_t ws_bytes = pick_ws_bytes(w, h, size_d);
    DevBuf dI, dC, dBest, dMap, dMean, dKeys, dAgg, ws;
    SMX_HIP(dI.alloc(n));
    SMX_HIP(dC.alloc(n * size_d * sizeof(float)));
    SMX_HIP(dBest.alloc(n * sizeof(float)));
    SMX_HIP(dMap.alloc(n * sizeof(float)));
    SMX_HIP(dMean.alloc(n));
    SMX_HIP(dKeys.alloc(n * sizeof(int64_t)));
    if (agg) SMX_HIP(dAgg.alloc(n * size_d * sizeof(float)));
    SMX_HIP(ws.alloc(ws_bytes));
    SMX_HIP(hipMemcpy(dI.p, i, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dC.p, cost, n * size_d * sizeof(float), hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dBest.p, filter_cost, n * sizeof(float), hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dMap.p, disp_map, n * sizeof(float), hipMemcpyHostToDevice));
    int rc;
    if ((rc = smx_dev_init_keys(dKeys.as<int64_t>(), (int64_t)n, nullptr))) return rc;
    if ((rc = smx_dev_aggregate_wta(p, dI.as<uint8_t>(), nullptr, dC.as<float>(), w, h, dmin, 0,
                                    size_d, dKeys.as<int64_t>(), dMean.as<uint8_t>(),
                                    agg ? dAgg.as<float>() : nullptr, ws.p, ws_bytes, nullptr)))
        return rc;
    if ((rc = smx_dev_apply_keys(dKeys.as<int64_t>(), (int64_t)n, dmin, dBest.as<float>(),
                                 dMap.as<float>(), nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if ((rc = smx_dev_agg_status(ws.p))) return rc;
    SMX_HIP(hipMemcpy(filter_cost, dBest.p, n * sizeof(float), hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(disp_map, dMap.p, n * sizeof(float), hipMemcpyDeviceToHost));
    if (mean) SMX_HIP(hipMemcpy(mean, dMean.p, n, hipMemcpyDeviceToHost));
    if (agg) SMX_HIP(hipMemcpy(agg, dAgg.p, n * size_d * sizeof(float), hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_detect_occlusion(const smx_params* p, float* disparityLeft, const float* disparityRight,
                         int dOcclusion, int w, int h) {
    SMX_ARG(p && disparityLeft && disparityRight && w >= 1 && h >= 1);
    const size_t bytes = (size_t)w * h * sizeof(float);
    DevBuf dL, dR;
    SMX_HIP(dL.alloc(bytes));
    SMX_HIP(dR.alloc(bytes));
    SMX_HIP(hipMemcpy(dL.p, disparityLeft, bytes, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dR.p, disparityRight, bytes, hipMemcpyHostToDevice));
    int rc = smx_dev_detect_occlusion(p, dL.as<float>(), dR.as<float>(), dOcclusion, w, h, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(disparityLeft, dL.p, bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_fill_occlusion(float* disparity, int w, int h, float vMin) {
    SMX_ARG(disparity && w >= 1 && h >= 1);
    const size_t bytes = (size_t)w * h * sizeof(float);
    DevBuf d;
    SMX_HIP(d.alloc(bytes));
    SMX_HIP(hipMemcpy(d.p, disparity, bytes, hipMemcpyHostToDevice));
    int rc = smx_dev_fill_occlusion(d.as<float>(), w, h, vMin, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(disparity, d.p, bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- weighted-median refinement (not in the reference; smx_wmf.hip) ----------------------------------
void smx_default_wmf_params(smx_wmf_params* p) {
    if (!p) return;
    p->radius = 9; p->sigma_s = 9.0; p->sigma_c = 25.5;
}

static bool wmf_params_ok(const smx_wmf_params* p) {
    return p && p->radius >= 1 && p->radius <= 15 && isfinite(p->sigma_s) && p->sigma_s > 0 && isfinite(p->sigma_c) &&
           p->sigma_c > 0;
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

int smx_weighted_median(const smx_wmf_params* p, const uint8_t* guide, const float* disp, const float* select,
                        float* out, int w, int h, int dmin, int size_d) {
    SMX_ARG(wmf_params_ok(p) && guide && disp && out && w >= 1 && h >= 1);
    SMX_ARG(size_d >= 1 && size_d <= 4096 && (long long)dmin + size_d <= INT_MAX);
    SMX_ARG((const void*)out != (const void*)disp);
    const size_t n = (size_t)w * h, bytes = n * sizeof(float);
    DevBuf dG, dD, dS, dO;
    SMX_HIP(dG.alloc(n));
    SMX_HIP(dD.alloc(bytes));
    SMX_HIP(dO.alloc(bytes));
    if (select) SMX_HIP(dS.alloc(bytes));
    SMX_HIP(hipMemcpy(dG.p, guide, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(dD.p, disp, bytes, hipMemcpyHostToDevice));
    if (select) SMX_HIP(hipMemcpy(dS.p, select, bytes, hipMemcpyHostToDevice));
    int rc = smx_dev_weighted_median(p, dG.as<uint8_t>(), dD.as<float>(), select ? dS.as<float>() : nullptr,
                                     dO.as<float>(), w, h, dmin, size_d, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(out, dO.p, bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- speckle removal (not in the reference; smx_speckle.hip) -------------------------------------------
void smx_default_speckle_params(smx_speckle_params* p) {
    if (!p) return;
    p->max_size = 200; p->max_diff = 1.0f;
}

static bool speckle_params_ok(const smx_speckle_params* p) {
    return p && p->max_size >= 0 && isfinite(p->max_diff) && p->max_diff >= 0.0f;
}
static bool speckle_shape_ok(int w, int h) { return w >= 1 && h >= 1 && (long long)w * h < (1ll << 31); }

size_t smx_speckle_workspace_bytes(int w, int h) { return speckle_shape_ok(w, h) ? speckle_workspace_bytes(w, h) : 0; }

int smx_speckle_geometry(int* tile_cols, int* tile_rows) {
    SMX_ARG(tile_cols && tile_rows);
    speckle_tile(tile_cols, tile_rows);
    return SMX_OK;
}

int smx_dev_speckle_filter(const smx_speckle_params* p, const float* d_disp, float* d_out, int w, int h, float vmin,
                           float new_val, void* d_ws, size_t ws_bytes, void* stream) {
    SMX_ARG(speckle_params_ok(p) && d_disp && d_out && speckle_shape_ok(w, h));
    if (!d_ws || ws_bytes < speckle_workspace_bytes(w, h))
        return fail(SMX_E_WS, "smx_dev_speckle_filter: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0,
                    speckle_workspace_bytes(w, h));
    return launch_speckle_filter(p->max_size, p->max_diff, d_disp, d_out, w, h, vmin, new_val, d_ws, (hipStream_t)stream);
}

int smx_speckle_filter(const smx_speckle_params* p, const float* disp, float* out, int w, int h, float vmin,
                       float new_val) {
    SMX_ARG(speckle_params_ok(p) && disp && out && speckle_shape_ok(w, h));
    const size_t bytes = (size_t)w * h * sizeof(float), wsb = speckle_workspace_bytes(w, h);
    DevBuf dD, dW;
    SMX_HIP(dD.alloc(bytes));
    SMX_HIP(dW.alloc(wsb));
    SMX_HIP(hipMemcpy(dD.p, disp, bytes, hipMemcpyHostToDevice));
    int rc = smx_dev_speckle_filter(p, dD.as<float>(), dD.as<float>(), w, h, vmin, new_val, dW.p, wsb, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(out, dD.p, bytes, hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- census / Hamming matching cost (not in the reference; smx_census.hip) ----------------------------
void smx_default_census_params(smx_census_params* p) {
    if (!p) return;
    p->rx = 4; p->ry = 3; p->th = 62;
}

static bool census_params_ok(const smx_census_params* p) {
    return p && p->rx >= 1 && p->rx <= 4 && p->ry >= 1 && p->ry <= 3 && p->th >= 1;
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

int smx_census_cost(const smx_census_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h,
                    int size_d, int dmin) {
    SMX_ARG(census_params_ok(p) && i1 && i2 && cost && w >= 1 && h >= 1 && size_d >= 1);
    const size_t n = (size_t)w * h;
    DevBuf img, code, dc;
    SMX_HIP(img.alloc(2 * n));
    SMX_HIP(code.alloc(2 * n * sizeof(uint64_t)));
    SMX_HIP(dc.alloc(n * size_d * sizeof(float)));
    SMX_HIP(hipMemcpy(img.p, i1, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + n, i2, n, hipMemcpyHostToDevice));
    int rc;
    if ((rc = smx_dev_census(p, img.as<uint8_t>(), code.as<uint64_t>(), w, h, 2, nullptr))) return rc;
    if ((rc = smx_dev_census_cost_pair(p, code.as<uint64_t>(), dc.as<float>(), nullptr, w, h, dmin, 0, 0, size_d, nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(cost, dc.p, n * size_d * sizeof(float), hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- semi-global matching (not in the reference; smx_sgm.hip) -----------------------------------------
void smx_default_sgm_params(smx_sgm_params* p) {
    if (!p) return;
    p->p1 = 10; p->p2 = 120; p->paths = 8;
}

static bool sgm_params_ok(const smx_sgm_params* p) {
    return p && p->p1 >= 0 && p->p1 <= p->p2 && p->p2 <= 4095 && (p->paths == 4 || p->paths == 8);
}
static bool sgm_shape_ok(int w, int h, int size_d) {
    return w >= 1 && h >= 1 && (long long)w * h < (1ll << 31) && size_d >= 1 && size_d <= SMX_SGM_MAX_D;
}

size_t smx_sgm_workspace_bytes(int w, int h, int size_d, int nviews) {
    return sgm_shape_ok(w, h, size_d) && (nviews == 1 || nviews == 2) ? sgm_workspace_bytes(w, h, size_d, nviews) : 0;
}

int smx_dev_sgm_wta_pair(const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                         int64_t* d_keys, float* d_agg, float* d_nbr, void* d_ws, size_t ws_bytes, void* stream) {
    if (!sgm_params_ok(p))
        return fail(SMX_E_ARG, "smx_dev_sgm_wta_pair: needs 0 <= p1 <= p2 <= 4095 and paths 4 or 8");
    if (!sgm_shape_ok(w, h, size_d))
        return fail(SMX_E_ARG, "smx_dev_sgm_wta_pair: needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= %d", SMX_SGM_MAX_D);
    SMX_ARG((d_cost_l || d_cost_r) && d_keys);
    const size_t need = sgm_workspace_bytes(w, h, size_d, d_cost_l && d_cost_r ? 2 : 1);
    if (!d_ws || ws_bytes < need)
        return fail(SMX_E_WS, "smx_dev_sgm_wta_pair: workspace of %zu bytes, %zu needed", d_ws ? ws_bytes : (size_t)0, need);
    return launch_sgm_wta_pair(p->p1, p->p2, p->paths, d_cost_l, d_cost_r, w, h, size_d, d_keys, d_agg, d_nbr, d_ws,
                               (hipStream_t)stream);
}

int smx_sgm_aggregate(const smx_sgm_params* p, const float* cost, float* agg, float* best, float* disp_map, int w, int h,
                      int size_d, int dmin) {
    if (!sgm_params_ok(p)) return fail(SMX_E_ARG, "smx_sgm_aggregate: needs 0 <= p1 <= p2 <= 4095 and paths 4 or 8");
    if (!sgm_shape_ok(w, h, size_d))
        return fail(SMX_E_ARG, "smx_sgm_aggregate: needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= %d", SMX_SGM_MAX_D);
    SMX_ARG(cost != nullptr);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float), wsb = sgm_workspace_bytes(w, h, size_d, 1);
    DevBuf dC, dA, dK, dW;
    SMX_HIP(dC.alloc(vb));
    if (agg) SMX_HIP(dA.alloc(vb));
    SMX_HIP(dK.alloc(n * sizeof(int64_t)));
    SMX_HIP(dW.alloc(wsb));
    SMX_HIP(hipMemcpy(dC.p, cost, vb, hipMemcpyHostToDevice));
    int rc = smx_dev_sgm_wta_pair(p, dC.as<float>(), nullptr, w, h, size_d, dK.as<int64_t>(), agg ? dA.as<float>() : nullptr,
                                  nullptr, dW.p, wsb, nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (agg) SMX_HIP(hipMemcpy(agg, dA.p, vb, hipMemcpyDeviceToHost));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(hipMemcpy(keys.data(), dK.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_dev_filter(const smx_params* p, const uint8_t* d_image, int w, int h, uint8_t* d_mean,
                   float* d_var, void* stream) {
    SMX_ARG(p && d_image && d_mean && d_var && w >= 1 && h >= 1 && p->radius >= 0);
    return launch_filter(p, d_image, d_mean, d_var, w, h, (hipStream_t)stream);
}

int smx_filter(const smx_params* p, const uint8_t* image, int w, int h, uint8_t* mean, float* var) {
    SMX_ARG(p && image && mean && var && w >= 1 && h >= 1 && p->radius >= 0);
    const size_t n = (size_t)w * h;
    DevBuf dI, dM, dV;
    SMX_HIP(dI.alloc(n));
    SMX_HIP(dM.alloc(n));
    SMX_HIP(dV.alloc(n * sizeof(float)));
    SMX_HIP(hipMemcpy(dI.p, image, n, hipMemcpyHostToDevice));
    int rc = smx_dev_filter(p, dI.as<uint8_t>(), w, h, dM.as<uint8_t>(), dV.as<float>(), nullptr);
    if (rc) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(mean, dM.p, n, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(var, dV.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- persistent context of the host-pointer pair entry ---------------------------------------------
struct smx_ctx {
    smx_params p;
    int w = 0, h = 0, size_d = 0, dev = -1;
    int agg_path = 0;      // this context's aggregation path (smx_ctx_set_agg_path); starts as the creating thread's
    size_t n = 0, ws_bytes = 0;
    hipStream_t st = nullptr;
    // keys / best / dmap / mean: left view first, right view behind it (one buffer each)
    DevBuf dL, dR, keys, best, map, mean, occ, fil, ws, costL, costR, aggLR;
    // sub-pixel maps (smx_ctx_set_subpixel): neighbour state [2][3][h][w], maps [2][h][w] and [h][w], allocated on first use
    int subpix = 0;
    bool sub_valid = false;     // the maps belong to the last synchronous pair
    DevBuf nbr, sub, subf;
    // census matching cost (smx_ctx_set_cost): the codes of both images [2][h][w] and, unless the whole volumes exist
    // (costL / costR), the cost slices of one chunk of both views [2][census_chunk][h][w]; allocated on first use
    int cost_mode = SMX_COST_REFERENCE;
    smx_census_params census;
    int census_chunk = 0;
    DevBuf codes, ccost;
    // speckle removal (smx_ctx_set_speckle): the despeckled left map [h][w] and the filter's workspace, allocated on first use
    bool speckle = false;
    bool spk_valid = false;     // the map belongs to the last synchronous pair
    smx_speckle_params spk_params;
    DevBuf spk, spk_ws;
    // semi-global matching (smx_ctx_set_aggregation): its workspace for both views, allocated on first use; the whole cost
    // volumes it reads are costL / costR
    int agg_mode = SMX_AGG_GUIDED;
    smx_sgm_params sgm;
    DevBuf sgm_ws;
    // pipelined entry (smx_ctx_stereo_pair_async): two slots of device inputs / results and pinned host staging, created
    // on first use.  Staging of a slot: [gray_l | gray_r] going up; [best_l best_r dmap_l dmap_r occlusion filled | mean_l
    // mean_r | status word] coming down.
    struct Slot {
        DevBuf in, res, mean;
        uint8_t* h_in = nullptr;
        char* h_out = nullptr;
        hipEvent_t up = nullptr, done = nullptr, down = nullptr;
        int dminl = 0, dminr = 0;
        bool busy = false;
    } slot[2];
    hipStream_t st_up = nullptr, st_dn = nullptr;
    uint64_t submitted = 0, waited = 0;
    ~smx_ctx() {
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

int smx_create(const smx_params* p, int w, int h, int size_d, smx_ctx** out) {
    SMX_ARG(p && out && w >= 2 && h >= 1 && size_d >= 1 && p->radius >= 0);
    *out = nullptr;
    smx_ctx* c = new (std::nothrow) smx_ctx;
    if (!c) return fail(SMX_E_HIP, "smx_create: out of host memory");
    struct Guard { smx_ctx* c; ~Guard() { delete c; } } guard{c};
    c->p = *p; c->w = w; c->h = h; c->size_d = size_d;
    c->agg_path = g_agg_path;
    c->n = (size_t)w * h;
    const size_t n = c->n, fb = n * sizeof(float);
    SMX_HIP(hipGetDevice(&c->dev));
    SMX_HIP(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    c->ws_bytes = 2 * pick_ws_bytes(w, h, size_d);     // both views per launch
    SMX_HIP(c->dL.alloc(n)); SMX_HIP(c->dR.alloc(n));
    SMX_HIP(c->keys.alloc(2 * n * 8));
    SMX_HIP(c->best.alloc(2 * fb)); SMX_HIP(c->map.alloc(2 * fb));
    SMX_HIP(c->mean.alloc(2 * n));
    SMX_HIP(c->occ.alloc(fb)); SMX_HIP(c->fil.alloc(fb));
    SMX_HIP(c->ws.alloc(c->ws_bytes));
    guard.c = nullptr;
    *out = c;
    return SMX_OK;
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

// Census mode of ctx_enqueue: the codes once per pair, then census cost chunk -> aggregation from that chunk over ascending
// contiguous chunks of `call`'s slices.  The chunk's slices go into the whole volumes where the context holds them, else
// into the chunk buffer.  Only the first chunk may take the thread's keys as fresh (the later ones accumulate into them).
static int ctx_census_aggregate(smx_ctx* c, const AggCall& call, bool whole) {
    const int w = c->w, h = c->h;
    const size_t n = c->n;
    hipStream_t st = call.st;
    uint64_t* codes = c->codes.as<uint64_t>();
    int rc;
    if (call.guide[1] == call.guide[0] + n) {
        if ((rc = smx_dev_census(&c->census, call.guide[0], codes, w, h, 2, st))) return rc;
    } else {
        for (int v = 0; v < 2; ++v)
            if ((rc = smx_dev_census(&c->census, call.guide[v], codes + v * n, w, h, 1, st))) return rc;
    }
    const int chunk = whole ? c->size_d : c->census_chunk;
    struct Fresh { int saved; Fresh() : saved(g_keys_fresh) {} ~Fresh() { g_keys_fresh = saved; } } fresh;
    for (int s0 = call.s_begin; s0 < call.s_end; s0 += chunk) {
        const int s1 = s0 + chunk < call.s_end ? s0 + chunk : call.s_end;
        float* cl = whole ? c->costL.as<float>() + (size_t)s0 * n : c->ccost.as<float>();
        float* cr = whole ? c->costR.as<float>() + (size_t)s0 * n : cl + (size_t)chunk * n;
        if ((rc = smx_dev_census_cost_pair(&c->census, codes, cl, cr, w, h, call.dmin[0], call.dmin[1], s0, s1, st))) return rc;
        AggCall part = call;
        part.s_begin = s0; part.s_end = s1;
        part.cost[0] = cl; part.cost[1] = cr;
        for (int v = 0; v < 2; ++v)
            if (call.agg[v]) part.agg[v] = call.agg[v] + (size_t)(s0 - call.s_begin) * n;
        if ((rc = run_aggregation(part, c->agg_path))) return rc;
        g_keys_fresh = 0;
    }
    return SMX_OK;
}

// SGM mode of ctx_enqueue with the census cost: the codes, then both whole volumes, in one launch each.
static int ctx_census_volumes(smx_ctx* c, const AggCall& call) {
    const size_t n = c->n;
    uint64_t* codes = c->codes.as<uint64_t>();
    int rc;
    for (int v = 0; v < 2; ++v)
        if ((rc = smx_dev_census(&c->census, call.guide[v], codes + v * n, c->w, c->h, 1, call.st))) return rc;
    return smx_dev_census_cost_pair(&c->census, codes, c->costL.as<float>(), c->costR.as<float>(), c->w, c->h, call.dmin[0],
                                    call.dmin[1], 0, c->size_d, call.st);
}

// The path of one pair on the context's stream: device images in, the eight result planes out (+ the optional volumes
// of the context).  Shared by the synchronous and the pipelined host-pointer entry.
static int ctx_enqueue(smx_ctx* c, const uint8_t* dL, const uint8_t* dR, int dminl, int dminr, bool want_cost, bool want_agg,
                       float* bestL, float* mapL, uint8_t* mean, float* occ, float* fil, bool subpix = false) {
    const smx_params* p = &c->p;
    const int w = c->w, h = c->h, size_d = c->size_d;
    const size_t n = c->n;
    hipStream_t st = c->st;
    int rc;
    const int64_t nn = (int64_t)n;
    int64_t* keysL = c->keys.as<int64_t>(); int64_t* keysR = keysL + n;
    // cost volumes are materialised only when the caller asks for them (main.cu:80-82) and then feed
    // the aggregation like in the reference; otherwise the slices are built on the fly inside it.
    const bool census = c->cost_mode == SMX_COST_CENSUS;
    const bool sgm = c->agg_mode == SMX_AGG_SGM;
    if (sgm) want_cost = true;      // SGM reads whole volumes
    if (want_cost && !census) {
        if ((rc = smx_dev_cost_volume(p, dL, dR, c->costL.as<float>(), w, w, h, dminl, 0, size_d, st))) return rc;
        if ((rc = smx_dev_cost_volume(p, dR, dL, c->costR.as<float>(), w, w, h, dminr, 0, size_d, st))) return rc;
    }
    if ((rc = smx_dev_init_keys(keysL, 2 * nn, st))) return rc;
    // main.cu:133-134, both views per call, on the context's own path
    float* const costL = want_cost ? c->costL.as<float>() : nullptr;
    float* const costR = want_cost ? c->costR.as<float>() : nullptr;
    float* const aggL = want_agg ? c->aggLR.as<float>() : nullptr;
    float* const nbrL = subpix ? c->nbr.as<float>() : nullptr;
    const AggCall call = {"smx_ctx_stereo_pair", p, 2, {dL, dR}, {dR, dL}, {costL, costR}, {dminl, dminr}, {keysL, keysR},
                          {mean, mean + n}, {aggL, want_agg ? aggL + (size_t)size_d * n : nullptr},
                          {nbrL, subpix ? nbrL + 3 * n : nullptr}, w, h, 0, size_d, c->ws.p, c->ws_bytes, st};
    if (sgm) {
        if (census) rc = ctx_census_volumes(c, call);
        if (!rc)
            rc = smx_dev_sgm_wta_pair(&c->sgm, costL, costR, w, h, size_d, keysL, aggL, nbrL, c->sgm_ws.p,
                                      sgm_workspace_bytes(w, h, size_d, 2), st);
    } else if (census) rc = ctx_census_aggregate(c, call, want_cost);
    else rc = run_aggregation(call, c->agg_path);
    if (rc) return rc;
    // main.cu:112-118 presets, winning slices, main.cu:140-155
    if ((rc = smx_dev_finish_pair(p, keysL, w, h, dminl, dminr, dminl - 100, (float)dminl, bestL, mapL, occ, fil, st))) return rc;
    const float* kept = occ;        // the map whose validity test says which pixels the fill replaced
    if (c->speckle) {
        // the small components of the LR-checked map join the invalidated pixels; the fill starts over from that map
        float* spk = c->spk.as<float>();
        if ((rc = smx_dev_speckle_filter(&c->spk_params, occ, spk, w, h, (float)dminl, (float)(dminl - 100), c->spk_ws.p,
                                         speckle_workspace_bytes(w, h), st)))
            return rc;
        if ((rc = launch_fill_occlusion(spk, fil, w, h, (float)dminl, st))) return rc;
        kept = spk;
    }
    if (!subpix) return SMX_OK;
    return smx_dev_subpixel_pair(c->subpix, keysL, c->nbr.as<float>(), mapL, kept, fil, w, h, dminl, c->sub.as<float>(),
                                 c->subf.as<float>(), st);
}

static int ctx_check_device(smx_ctx* c, const char* who) {
    int dev = -1;
    SMX_HIP(hipGetDevice(&dev));
    if (dev != c->dev) return fail(SMX_E_ARG, "%s: the context lives on device %d, current device is %d", who, c->dev, dev);
    return SMX_OK;
}

int smx_ctx_stereo_pair(smx_ctx* c, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr,
                        const smx_pair_out* out) {
    SMX_ARG(c && gray_l && gray_r && out);
    const int size_d = c->size_d;
    const size_t n = c->n, fb = n * sizeof(float), vb = fb * size_d;
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_stereo_pair"))) return rc;
    if (c->submitted != c->waited) return fail(SMX_E_ARG, "smx_ctx_stereo_pair: pipelined pairs are still in flight (smx_ctx_wait)");
    hipStream_t st = c->st;
    const bool sgm = c->agg_mode == SMX_AGG_SGM;
    if (sgm && (out->mean_l || out->mean_r))
        return fail(SMX_E_ARG, "smx_ctx_stereo_pair: semi-global matching (smx_ctx_set_aggregation) produces no mean images");
    const bool want_cost = out->cost_l || out->cost_r || sgm;
    const bool want_agg = out->agg_l || out->agg_r;
    if (sgm && !c->sgm_ws.p) SMX_HIP(c->sgm_ws.alloc(sgm_workspace_bytes(c->w, c->h, size_d, 2)));
    if (want_cost && !c->costL.p) { SMX_HIP(c->costL.alloc(vb)); SMX_HIP(c->costR.alloc(vb)); }
    if (want_agg && !c->aggLR.p) SMX_HIP(c->aggLR.alloc(2 * vb));
    const bool subpix = c->subpix != 0;
    if (subpix && !c->nbr.p) { SMX_HIP(c->nbr.alloc(6 * fb)); SMX_HIP(c->sub.alloc(2 * fb)); SMX_HIP(c->subf.alloc(fb)); }
    if (c->cost_mode == SMX_COST_CENSUS) {
        if (!c->codes.p) SMX_HIP(c->codes.alloc(2 * n * sizeof(uint64_t)));
        if (!want_cost && !c->ccost.p) {     // (SGM takes whole volumes: no chunk buffer)
            // at most 1 GiB for the chunk's two cost buffers
            const size_t fit = ((size_t)1 << 30) / (2 * fb);
            c->census_chunk = (int)(fit < 1 ? 1 : fit > (size_t)size_d ? (size_t)size_d : fit);
            SMX_HIP(c->ccost.alloc(2 * (size_t)c->census_chunk * fb));
        }
    }
    if (c->speckle && !c->spk.p) { SMX_HIP(c->spk.alloc(fb)); SMX_HIP(c->spk_ws.alloc(speckle_workspace_bytes(c->w, c->h))); }
    c->sub_valid = false;
    c->spk_valid = false;
    uint8_t* dL = c->dL.as<uint8_t>(); uint8_t* dR = c->dR.as<uint8_t>();
    stage_mark(ST_BEGIN, st);
    SMX_HIP(hipMemcpyAsync(dL, gray_l, n, hipMemcpyHostToDevice, st));
    SMX_HIP(hipMemcpyAsync(dR, gray_r, n, hipMemcpyHostToDevice, st));
    stage_mark(ST_UPLOAD, st);
    float* bestL = c->best.as<float>(); float* bestR = bestL + n;
    float* mapL = c->map.as<float>();   float* mapR = mapL + n;
    if ((rc = ctx_enqueue(c, dL, dR, dminl, dminr, want_cost, want_agg, bestL, mapL, c->mean.as<uint8_t>(), c->occ.as<float>(),
                          c->fil.as<float>(), subpix)))
        return rc;
    struct { void* dst; const void* src; size_t b; } copies[] = {
        {out->best_l, bestL, fb}, {out->best_r, bestR, fb}, {out->dmap_l, mapL, fb},
        {out->dmap_r, mapR, fb},  {out->mean_l, c->mean.p, n}, {out->mean_r, c->mean.as<uint8_t>() + n, n},
        {out->occlusion, c->occ.p, fb}, {out->filled, c->fil.p, fb},  {out->cost_l, c->costL.p, vb},
        {out->cost_r, c->costR.p, vb}, {out->agg_l, c->aggLR.p, vb},
        {out->agg_r, want_agg ? (const void*)(c->aggLR.as<float>() + (size_t)size_d * n) : nullptr, vb},
    };
    for (auto& cp : copies)
        if (cp.dst && cp.src) SMX_HIP(hipMemcpyAsync(cp.dst, cp.src, cp.b, hipMemcpyDeviceToHost, st));
    stage_mark(ST_DOWNLOAD, st);
    SMX_HIP(hipStreamSynchronize(st));
    if (!sgm && (rc = smx_dev_agg_status(c->ws.p))) return rc;      // (the SGM kernels wait for nothing)
    c->sub_valid = subpix;
    c->spk_valid = c->speckle;
    return SMX_OK;
}

int smx_ctx_set_subpixel(smx_ctx* c, int mode) {
    SMX_ARG(c);
    if (mode != 0 && !subpix_mode_ok(mode))
        return fail(SMX_E_ARG, "smx_ctx_set_subpixel: mode must be 0, SMX_SUBPIX_PARABOLA or SMX_SUBPIX_EQUIANGULAR");
    c->subpix = mode;
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
        if (!census_params_ok(&p))
            return fail(SMX_E_ARG, "smx_ctx_set_cost: census needs 1 <= rx <= 4, 1 <= ry <= 3, th >= 1");
        c->census = p;
    }
    c->cost_mode = mode;
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
        if (!sgm_params_ok(&p))
            return fail(SMX_E_ARG, "smx_ctx_set_aggregation: SGM needs 0 <= p1 <= p2 <= 4095 and paths 4 or 8");
        if (!sgm_shape_ok(c->w, c->h, c->size_d))
            return fail(SMX_E_ARG, "smx_ctx_set_aggregation: SGM needs w*h < 2^31 and size_d <= %d", SMX_SGM_MAX_D);
        c->sgm = p;
    }
    c->agg_mode = mode;
    return SMX_OK;
}

int smx_ctx_set_speckle(smx_ctx* c, const smx_speckle_params* p) {
    SMX_ARG(c);
    if (p) {
        if (!speckle_params_ok(p))
            return fail(SMX_E_ARG, "smx_ctx_set_speckle: needs max_size >= 0 and a finite max_diff >= 0");
        if (!speckle_shape_ok(c->w, c->h)) return fail(SMX_E_ARG, "smx_ctx_set_speckle: needs w*h < 2^31");
        c->spk_params = *p;
    }
    c->speckle = p != nullptr;
    return SMX_OK;
}

int smx_ctx_speckle_map(smx_ctx* c, float* despeckled) {
    SMX_ARG(c);
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_speckle_map"))) return rc;
    if (!c->spk_valid) return fail(SMX_E_ARG, "smx_ctx_speckle_map: the last smx_ctx_stereo_pair ran without speckle removal");
    if (despeckled) SMX_HIP(hipMemcpy(despeckled, c->spk.p, c->n * sizeof(float), hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_ctx_subpixel_maps(smx_ctx* c, float* sub_l, float* sub_r, float* sub_filled) {
    SMX_ARG(c);
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_subpixel_maps"))) return rc;
    if (!c->sub_valid) return fail(SMX_E_ARG, "smx_ctx_subpixel_maps: the last smx_ctx_stereo_pair ran without sub-pixel");
    const size_t n = c->n, fb = n * sizeof(float);
    if (sub_l) SMX_HIP(hipMemcpy(sub_l, c->sub.p, fb, hipMemcpyDeviceToHost));
    if (sub_r) SMX_HIP(hipMemcpy(sub_r, c->sub.as<float>() + n, fb, hipMemcpyDeviceToHost));
    if (sub_filled) SMX_HIP(hipMemcpy(sub_filled, c->subf.p, fb, hipMemcpyDeviceToHost));
    return SMX_OK;
}

// ---- pipelined host-pointer entry ---------------------------------------------------------------------------------
// Pair k uses slot k % 2.  Three streams: uploads, the path, downloads; events chain a pair through them, so that the
// upload of pair k+1 and the download of pair k-1 run under the aggregation of pair k.
static size_t slot_out_bytes(size_t n) { return 6 * n * sizeof(float) + 2 * n + 256; }

static int ctx_async_setup(smx_ctx* c) {
    if (c->st_up) return SMX_OK;
    const size_t n = c->n;
    SMX_HIP(hipStreamCreateWithFlags(&c->st_up, hipStreamNonBlocking));
    SMX_HIP(hipStreamCreateWithFlags(&c->st_dn, hipStreamNonBlocking));
    for (smx_ctx::Slot& sl : c->slot) {
        SMX_HIP(sl.in.alloc(2 * n));
        SMX_HIP(sl.res.alloc(6 * n * sizeof(float)));
        SMX_HIP(sl.mean.alloc(2 * n));
        SMX_HIP(hipHostMalloc((void**)&sl.h_in, 2 * n, hipHostMallocDefault));
        SMX_HIP(hipHostMalloc((void**)&sl.h_out, slot_out_bytes(n), hipHostMallocDefault));
        SMX_HIP(hipEventCreateWithFlags(&sl.up, hipEventDisableTiming));
        SMX_HIP(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        SMX_HIP(hipEventCreateWithFlags(&sl.down, hipEventDisableTiming));
    }
    return SMX_OK;
}

int smx_ctx_stereo_pair_async(smx_ctx* c, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr) {
    SMX_ARG(c && gray_l && gray_r);
    int rc;
    if ((rc = ctx_check_device(c, "smx_ctx_stereo_pair_async"))) return rc;
    if (c->subpix) return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: sub-pixel is on (smx_ctx_set_subpixel): use smx_ctx_stereo_pair");
    if (c->speckle) return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: speckle removal is on (smx_ctx_set_speckle): use smx_ctx_stereo_pair");
    if (c->agg_mode != SMX_AGG_GUIDED)
        return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: semi-global matching is on (smx_ctx_set_aggregation): use smx_ctx_stereo_pair");
    if (c->cost_mode != SMX_COST_REFERENCE)
        return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: the census cost is on (smx_ctx_set_cost): use smx_ctx_stereo_pair");
    if (c->submitted - c->waited >= 2)
        return fail(SMX_E_ARG, "smx_ctx_stereo_pair_async: two pairs are in flight already (smx_ctx_wait takes the older one)");
    if ((rc = ctx_async_setup(c))) return rc;
    // no stage marks in the pipelined entry: pairs overlap on three streams, so "the stages of the last call" has no meaning
    // here, and an event record per stage is a bubble on the queue the pipeline exists to keep full
    struct Pause { int saved; Pause() : saved(g_timing) { g_timing = 0; } ~Pause() { g_timing = saved; } } pause;
    const size_t n = c->n, fb = n * sizeof(float);
    smx_ctx::Slot& sl = c->slot[c->submitted & 1];
    // the caller's images into the slot's pinned staging: the caller's buffers are free again when this call returns
    memcpy(sl.h_in, gray_l, n);
    memcpy(sl.h_in + n, gray_r, n);
    sl.dminl = dminl; sl.dminr = dminr;
    uint8_t* dL = sl.in.as<uint8_t>(); uint8_t* dR = dL + n;
    SMX_HIP(hipMemcpyAsync(dL, sl.h_in, 2 * n, hipMemcpyHostToDevice, c->st_up));
    SMX_HIP(hipEventRecord(sl.up, c->st_up));
    SMX_HIP(hipStreamWaitEvent(c->st, sl.up, 0));
    float* r = sl.res.as<float>();                       // best_l best_r dmap_l dmap_r occlusion filled
    if ((rc = ctx_enqueue(c, dL, dR, dminl, dminr, false, false, r, r + 2 * n, sl.mean.as<uint8_t>(), r + 4 * n, r + 5 * n)))
        return rc;
    // status word of this pair's aggregation (the next pair's launch clears it): behind the planes in the staging
    char* status_h = sl.h_out + 6 * fb + 2 * n;
    SMX_HIP(hipMemcpyAsync(status_h, (const char*)align_up((size_t)c->ws.p, 256), sizeof(unsigned), hipMemcpyDeviceToHost, c->st));
    SMX_HIP(hipEventRecord(sl.done, c->st));
    SMX_HIP(hipStreamWaitEvent(c->st_dn, sl.done, 0));
    SMX_HIP(hipMemcpyAsync(sl.h_out, r, 6 * fb, hipMemcpyDeviceToHost, c->st_dn));
    SMX_HIP(hipMemcpyAsync(sl.h_out + 6 * fb, sl.mean.p, 2 * n, hipMemcpyDeviceToHost, c->st_dn));
    SMX_HIP(hipEventRecord(sl.down, c->st_dn));
    sl.busy = true;
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
    sl.busy = false;
    ++c->waited;
    const size_t n = c->n, fb = n * sizeof(float);
    float* f = (float*)sl.h_out;
    uint8_t* m = (uint8_t*)(sl.h_out + 6 * fb);
    smx_pair_out v;
    memset(&v, 0, sizeof(v));
    v.best_l = f; v.best_r = f + n; v.dmap_l = f + 2 * n; v.dmap_r = f + 3 * n; v.occlusion = f + 4 * n; v.filled = f + 5 * n;
    v.mean_l = m; v.mean_r = m + n;
    if (staged) *staged = v;
    if (copy_to) {
        struct { void* dst; const void* src; size_t b; } copies[] = {
            {copy_to->best_l, v.best_l, fb}, {copy_to->best_r, v.best_r, fb}, {copy_to->dmap_l, v.dmap_l, fb},
            {copy_to->dmap_r, v.dmap_r, fb}, {copy_to->occlusion, v.occlusion, fb}, {copy_to->filled, v.filled, fb},
            {copy_to->mean_l, v.mean_l, n}, {copy_to->mean_r, v.mean_r, n},
        };
        for (auto& cp : copies)
            if (cp.dst) memcpy(cp.dst, cp.src, cp.b);
    }
    unsigned status = 0;
    memcpy(&status, sl.h_out + 6 * fb + 2 * n, sizeof(status));
    if (status != 0)
        return fail(SMX_E_HIP, "fused aggregation: hand-off wait of work item %u timed out (results invalid)", status - 1);
    return SMX_OK;
}

int smx_stereo_pair(const smx_params* p, const uint8_t* gray_l, const uint8_t* gray_r, int w, int h,
                    int size_d, int dminl, int dminr, const smx_pair_out* out) {
    SMX_ARG(p && gray_l && gray_r && out && w >= 2 && h >= 1 && size_d >= 1);
    smx_ctx* c = nullptr;
    int rc = smx_create(p, w, h, size_d, &c);
    if (rc) return rc;
    rc = smx_ctx_stereo_pair(c, gray_l, gray_r, dminl, dminr, out);
    (void)smx_destroy(c);
    return rc;
}

}  // extern "C"
