/*
 * smx.h -- C-ABI of the MI355X (gfx950) stereo-pair -> disparity-map library
 *          (libsmx_hip.so, built from stereo_matching_cuda_amd/csrc/).
 *
 * This is the drop-in boundary for the one hot path of hamza1030/stereo_matching_cuda:
 *   gray -> cost volume -> guided-filter aggregation + winner-take-all -> LR check -> fill,
 * and, beyond the reference, an optional weighted-median refinement of the filled map (smx_weighted_median) and an
 * optional speckle filter in front of the fill (smx_speckle_filter).
 * Every entry point cites the reference host function it replaces (paths relative to the
 * reference's stereo_matching_cuda/ directory).  Plain pointers and sizes only.
 *
 * Two families:
 *   smx_<stage>()      host pointers in / host pointers out, synchronous -- exactly the
 *                      calling convention of the reference's per-stage wrappers, so the
 *                      reference-signature C++ functions in stereo_matching_cuda_amd/host/
 *                      (costVolume.cuh, guidedFilter.cuh, ...) are one-line forwards.
 *   smx_dev_<stage>()  device pointers, asynchronous on a caller-supplied hipStream_t
 *                      (passed as void*) of the CURRENT device, caller-supplied workspace; no
 *                      allocation, no synchronisation and no internal streams or events: a
 *                      call is a fixed sequence of kernel launches and small memsets on
 *                      `stream`, so a pair step can be captured into a hipGraph and replayed
 *                      (tests/test_gpu_parity.py::test_pair_step_is_capturable_in_a_hip_graph).
 *                      Used by the pair path, the benchmark and the multi-GPU (D-sharded)
 *                      drivers (sharded.py; include/smx_rccl.h).
 *
 * All functions return 0 on success or a negative code (SMX_E_*); smx_last_error() gives
 * the message of the last failure on the calling thread.  There is no CPU fallback: without
 * a HIP device every compute entry point fails with SMX_E_HIP.
 *
 * Layouts (reference: costVolume.cu:178, guidedFilter.cu:173,198): images row-major [y][x];
 * volumes [z][y][x] with plane stride w*h; disparity maps are float arrays holding integer
 * labels (dmin + slice index).
 */
#ifndef SMX_H
#define SMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define SMX_OK 0
#define SMX_E_ARG (-1)  /* bad argument (null pointer, non-positive size, ...) */
#define SMX_E_HIP (-2)  /* HIP runtime error or no device */
#define SMX_E_WS (-3)   /* workspace too small */

/* Tunables of the reference (SystemIncludes.h:7-24), runtime instead of macros. */
typedef struct smx_params {
    double r_w, g_w, b_w; /* R_W 0.299, G_W 0.587, B_W 0.0721 (sic)  SystemIncludes.h:7-9 */
    double alpha;         /* ALPHA 0.9                                :10 */
    int th_color;         /* TH_color 7                               :14 */
    int th_grad;          /* TH_grad 2                                :13 */
    int radius;           /* RADIUS 9                                 :21 */
    double eps;           /* EPS 6.5025                               :23 */
    int d_lr;             /* D_LR 0                                   :24 */
} smx_params;

void smx_default_params(smx_params* p);
const char* smx_last_error(void);
const char* smx_version(void);
/* Number of visible HIP devices (0 if none / runtime unusable). Never fails. */
int smx_device_count(void);

/* ------------------------------------------------------------------------------------
 * Host-pointer stage API (reference L2 wrappers)
 * ---------------------------------------------------------------------------------- */

/* rgb_to_grayscale.cuh:7  unsigned char* rgb_to_grayscale(h_rgb, n, channels, compare)
 * gray[k] = (uchar)(R_W*r + G_W*g + B_W*b) in double.  h_gray: caller-allocated, n bytes. */
int smx_rgb_to_grayscale(const smx_params* p, const uint8_t* h_rgb, int64_t n, int channels,
                         uint8_t* h_gray);

/* costVolume.cuh:7  void compute_cost(i1, i2, cost, w1, w2, h1, h2, dmin, compare)
 * size_d is explicit here (the reference derives it from macros, costVolume.cu:5).
 * cost: size_d*w1*h1 floats, [z][y][x], label of slice z = dmin + z. */
int smx_compute_cost(const smx_params* p, const uint8_t* i1, const uint8_t* i2, float* cost,
                     int w1, int w2, int h1, int h2, int size_d, int dmin);

/* integral.cuh:3  void integral(float* image, float* integral, int width, int height) */
int smx_integral(const float* image, float* integral, int width, int height);

/* guidedFilter.cuh:7  void compute_guided_filter(i, cost, filter_cost, disp_map, mean, w, h,
 *                                                size_d, dmin, compare)
 * filter_cost / disp_map are IN/OUT exactly as in the reference (main.cu:112-118 presets them
 * to 0x7F7F7F7F / 0): a pixel is updated iff filter_cost >= min_z q[z].  mean (u8, optional)
 * receives trunc(mean_I).  agg (optional, size_d*w*h floats) receives the aggregated volume q,
 * which the reference never materialises (guidedFilter.cu:233). */
int smx_compute_guided_filter(const smx_params* p, const uint8_t* i, const float* cost,
                              float* filter_cost, float* disp_map, uint8_t* mean, float* agg,
                              int w, int h, int size_d, int dmin);

/* occlusion.cuh:8  void detect_occlusion(dL, dR, dOcclusion, dmapl, dmapr, w, h)
 * (the two u8 arguments of the reference are dead: occlusion.cu:51-52). dL is in/out. */
int smx_detect_occlusion(const smx_params* p, float* disparityLeft, const float* disparityRight,
                         int dOcclusion, int w, int h);

/* occlusion.cuh:14  void fill_occlusion(float* disparity, w, h, vMin) ; in place.
 * One wave per row with the row staged in LDS: w <= 16384 (SMX_E_ARG above that). */
int smx_fill_occlusion(float* disparity, int w, int h, float vMin);

/* filter.cuh:12  void filter(image, width, height, mean, var, cuda)   (dead code in the reference:
 * never called from main.cu).  Direct (2R+1)^2 box filter with zero padding, truncated means:
 * mean = (uchar)(int)(sum(I)/(2R+1)^2); var = (float)(int)(sum(I*I)/(2R+1)^2) - mean*mean
 * (filter.cu:39-115, 143-181).  mean: w*h bytes, var: w*h floats, caller-allocated. */
int smx_filter(const smx_params* p, const uint8_t* image, int w, int h, uint8_t* mean, float* var);

/* main.cu:65-155 as one call on two gray images (device-resident between stages).
 * Left volume labels dminl .. dminl+size_d-1, right volume dminr .. dminr+size_d-1
 * (main.cu:79-82).  Any output pointer may be NULL.  occlusion uses dOcclusion = dminl-100
 * (main.cu:149) and filling uses vMin = dminl (main.cu:154). */
typedef struct smx_pair_out {
    float* best_l; float* best_r;   /* n floats each: WTA cost (main.cu best_costl/r)      */
    float* dmap_l; float* dmap_r;   /* n floats each: labels                                */
    uint8_t* mean_l; uint8_t* mean_r;
    float* occlusion;               /* left map after LR check                              */
    float* filled;                  /* after scan-line filling                              */
    float* cost_l; float* cost_r;   /* size_d*n floats each, raw cost volumes (optional)    */
    float* agg_l; float* agg_r;     /* size_d*n floats each, aggregated volumes (optional)  */
} smx_pair_out;

int smx_stereo_pair(const smx_params* p, const uint8_t* gray_l, const uint8_t* gray_r, int w,
                    int h, int size_d, int dminl, int dminr, const smx_pair_out* out);

/* Persistent context for the host-pointer pair entry: device buffers, workspace and stream are created once
 * and reused by every pair of the same shape.  It replaces the per-call allocation churn of the reference's
 * wrappers (guidedFilter.cu:50-56,182-194: 13 planes uploaded per slice; integral.cu:3-51: five cudaMalloc /
 * cudaFree per call), which smx_stereo_pair still pays once per call (it is smx_create + smx_ctx_stereo_pair +
 * smx_destroy).  The context belongs to the device that was current at smx_create; use it from one host thread
 * at a time.  cost_* / agg_* volumes are allocated on first request and kept. */
typedef struct smx_ctx smx_ctx;
int smx_create(const smx_params* p, int w, int h, int size_d, smx_ctx** ctx);
int smx_ctx_stereo_pair(smx_ctx* ctx, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr,
                        const smx_pair_out* out);
int smx_destroy(smx_ctx* ctx);
/* Pipelined host-pointer entry: uploads of pair k+1 and downloads of pair k-1 run under the aggregation of pair k
 * (three streams, pinned staging buffers owned by the context; it replaces the synchronous per-slice upload / compute /
 * download churn of guidedFilter.cu:50-56,182-194,244-248).
 *   smx_ctx_stereo_pair_async  copies the two images into pinned staging (the caller's buffers are free when it returns),
 *                              enqueues upload -> path -> download of the eight result planes and returns without
 *                              waiting.  At most two pairs may be in flight (SMX_E_ARG otherwise).
 *   smx_ctx_wait               waits for the OLDEST pair in flight.  `staged` (may be NULL) receives pointers to its
 *                              results inside the context's pinned staging -- valid until two more pairs have been
 *                              submitted; `copy_to` (may be NULL) names caller buffers the planes are copied into as
 *                              well (a host memcpy of 26 bytes per pixel: use `staged` where the rate matters).
 *                              cost_* / agg_* volumes are not part of the pipelined entry.  Returns the pair's status.
 * Results equal those of smx_ctx_stereo_pair bit for bit.  The synchronous entry refuses to run while pairs are in flight. */
int smx_ctx_stereo_pair_async(smx_ctx* ctx, const uint8_t* gray_l, const uint8_t* gray_r, int dminl, int dminr);
int smx_ctx_wait(smx_ctx* ctx, smx_pair_out* staged, const smx_pair_out* copy_to);
/* Aggregation path of this context (ids as for smx_set_agg_path below). */
int smx_ctx_set_agg_path(smx_ctx* ctx, int path);
/* Sub-pixel disparity of this context (smx_dev_subpixel_pair below): mode 0 off (the default), SMX_SUBPIX_PARABOLA or
 * SMX_SUBPIX_EQUIANGULAR.  The state and map buffers are allocated on first use.  While it is on, smx_ctx_stereo_pair
 * aggregates through the _nbr passes and computes the maps, and smx_ctx_stereo_pair_async returns SMX_E_ARG.
 * smx_ctx_subpixel_maps copies the maps of the last synchronous smx_ctx_stereo_pair of the context (n floats each; any
 * pointer may be NULL); SMX_E_ARG if that pair ran without sub-pixel.  No other output changes. */
int smx_ctx_set_subpixel(smx_ctx* ctx, int mode);
int smx_ctx_subpixel_maps(smx_ctx* ctx, float* sub_l, float* sub_r, float* sub_filled);

/* ------------------------------------------------------------------------------------
 * Device-pointer API (async on `stream`, no allocation inside)
 * ---------------------------------------------------------------------------------- */

int smx_dev_rgb_to_grayscale(const smx_params* p, const uint8_t* d_rgb, int64_t n, int channels,
                             uint8_t* d_gray, void* stream);

/* Slices [s_begin, s_end) of the volume whose slice z has label dmin+z are written to
 * d_cost[(z - s_begin) * w1*h]. */
int smx_dev_cost_volume(const smx_params* p, const uint8_t* d_i1, const uint8_t* d_i2,
                        float* d_cost, int w1, int w2, int h, int dmin, int s_begin, int s_end,
                        void* stream);

/* nplanes independent w*h planes, in place allowed (d_in == d_out). */
int smx_dev_integral(const float* d_in, float* d_out, int w, int h, int nplanes, void* stream);

/* Bytes of workspace smx_dev_aggregate_wta needs for `nslices` slices of ONE view in flight (the pair
 * call needs twice that): image / guidance planes, per slice one aggregated plane plus the strip
 * hand-off records, control words.  The first 256 bytes hold the call's status word
 * (smx_dev_agg_status).  Fewer slices in flight than s_end - s_begin only means more launches.
 *
 * The memory contract of the five aggregation entries (smx_dev_aggregate_wta, _pair, _pair_cost, _nbr, _pair_nbr;
 * tests/test_gpu_memory_contract.py) and of smx_dev_aggregate_wta_pair_uq (tests/test_gpu_uniq.py):
 *   - A call writes nothing outside [d_workspace, d_workspace + workspace_bytes) and the stated extents of its outputs:
 *     d_keys n keys per view, d_mean_u8 n bytes per view, d_agg (s_end - s_begin) * n floats per view, d_nbr 3n floats per
 *     view, d_uq 3n floats per view (n = w*h).  A workspace too small for one slice is SMX_E_WS before anything is launched or written.
 *   - The workspace may hold anything on entry: the call clears the status words, tickets and flags it relies on, and reads
 *     no other region before it has written it.
 *   - d_workspace needs no alignment: the call uses it from the next 256-byte boundary on, and the sizes below include the
 *     up to 255 bytes that loses.
 *   - Inputs (the images, d_cost*) are not modified. */
size_t smx_agg_workspace_bytes(int w, int h, int nslices);
/* The same for the path that `p` will run in auto mode: where a fused walker runs (radius <= 9, thresholds within the
 * sentinel bound below) it needs ONE plane per slice in flight (plus its hand-off records), about a quarter of the
 * parameter-agnostic bound above, which has to cover the five planes per slice of the multi-kernel path (radius > 9,
 * larger thresholds, or smx_set_agg_path(1)).  At 3840x2160 this is what lets all 512
 * slices of a volume go out in one launch inside 64 GB. */
size_t smx_agg_workspace_bytes_for(const smx_params* p, int w, int h, int nslices);

/* Guided-filter aggregation + running winner-take-all over slices [s_begin, s_end) of ONE
 * volume (reference: guidedFilter.cu:171-238 incl. dispSelectOnGPU :403-411).
 *   d_guide  : guidance image I (u8, w*h) -- the image the volume belongs to
 *   d_other  : the other view; used to build cost slices on the fly when d_cost == NULL
 *              (costVolume.cu:163-190 fused in).  May be NULL when d_cost is given.
 *   d_cost   : optional materialised cost slices, slice s at d_cost[(s - s_begin)*w*h]
 *   d_keys   : n packed WTA keys, IN/OUT: key = sord(cost)<<32 | (0xFFFFFFFF - slice) compared as
 *              signed 64-bit integers (sord = order-preserving f32 -> i32 map); initialise with
 *              smx_dev_init_keys (INT64_MAX); combine across shards with an int64 MIN all-reduce
 *   d_mean_u8: optional u8 mean image out (guidedFilter.cu:87,122)
 *   d_agg    : optional aggregated slices out, slice s at d_agg[(s - s_begin)*w*h]; any 4-byte aligned pointer
 *              (the WTA pass reads it with 8-byte loads when it is 8-byte aligned and w*h is even, else with 4-byte ones)
 * Slices are processed in chunks that fit the workspace (>= smx_agg_workspace_bytes(w,h,1)). */
int smx_dev_aggregate_wta(const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                          const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                          int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* Both views of a stereo pair in one call (main.cu:133-134 back to back): every kernel launch
 * covers the left and the right volume.  View 0 = left (guide d_left, labels dminl + s), view 1 = right (guide d_right, labels
 * dminr + s).  d_keys: 2*n keys (left then right); d_mean_u8: NULL or 2*n bytes; d_agg: NULL or two
 * volumes of (s_end - s_begin)*n floats.  Workspace: >= 2 * smx_agg_workspace_bytes(w, h, nslices). */
int smx_dev_aggregate_wta_pair(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                               int w, int h, int dminl, int dminr, int s_begin, int s_end,
                               int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                               size_t workspace_bytes, void* stream);

/* The same with the two cost volumes materialised by the caller -- main.cu:80-82 followed by main.cu:133-134, i.e. the
 * reference's own data flow: read the raw cost, write / consume the aggregated cost (guidedFilter.cu:198-233).  Slice s of a
 * volume at d_cost_*[(s - s_begin) * w*h], as for smx_dev_aggregate_wta. */
int smx_dev_aggregate_wta_pair_cost(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                    const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                    int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                    void* d_workspace, size_t workspace_bytes, void* stream);

/* Sub-pixel refinement (not a stage of the reference; opt-in).  The _nbr forms of the aggregation calls also keep, per
 * pixel, the aggregated costs of the running winner's neighbouring slices, in a state d_nbr of three f32 planes per view
 * [3][h][w]: 0 lo = the cost of the slice just before the winner, 1 hi = the cost of the slice just after it, 2 last = the
 * cost of the last slice the view has aggregated.  Keys and winners are those of the plain calls, bit for bit.
 *   - d_nbr is IN/OUT like d_keys: 3*n floats (smx_dev_aggregate_wta_nbr) or 6*n, left view first
 *     (smx_dev_aggregate_wta_pair_nbr); it needs no initialisation -- a pixel whose key is the identity (fresh keys,
 *     smx_dev_init_keys) starts without state.
 *   - Calls on one set of keys must cover ascending, contiguous slice ranges.  A neighbour outside the slices aggregated
 *     so far is unknown (NaN): hi of a winner at the last slice so far, lo of a winner at the first slice of the first call.
 *     A pixel whose key stays the identity has lo = hi = NaN.
 *   - smx_dev_aggregate_wta_pair_nbr takes d_cost_l / d_cost_r both NULL (the _pair convention) or both set (_pair_cost).
 *   - Both honour smx_set_max_slices_per_launch and smx_set_keys_fresh like the plain calls; the workspace is the same.
 * The state is per volume: it does not combine across D-shards. */
int smx_dev_aggregate_wta_nbr(const smx_params* p, const uint8_t* d_guide, const uint8_t* d_other,
                              const float* d_cost, int w, int h, int dmin, int s_begin, int s_end,
                              int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg, void* d_workspace,
                              size_t workspace_bytes, float* d_nbr, void* stream);
int smx_dev_aggregate_wta_pair_nbr(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                   const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                   int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                   void* d_workspace, size_t workspace_bytes, float* d_nbr, void* stream);

#define SMX_SUBPIX_PARABOLA 1    /* delta = (a - b) / (2 (a + b)) */
#define SMX_SUBPIX_EQUIANGULAR 2 /* delta = (a - b) / (2 max(a, b)) */
/* The sub-pixel maps of a pair behind smx_dev_finish_pair, both views in one launch (no allocation: graph-capturable).
 * Per pixel of view v: c0 = the cost of its key, a = lo - c0, b = hi - c0 (f32), delta as above, and delta = 0 where the
 * key is the identity, lo or hi is NaN, or the result is not finite; d_sub[v*n + i] = d_dmap[v*n + i] + delta.  By the
 * tie rule (the last slice of equal costs wins) a >= 0 and b > 0, so |delta| <= 0.5.
 *   d_keys 2n, d_nbr 6n (the _pair_nbr state), d_dmap 2n (the finish's label maps), d_sub 2n floats out (not d_dmap).
 *   d_sub_filled: NULL, or n floats out for the left view: d_sub where the LR check kept the pixel, d_filled where it did
 *   not -- fill_occlusion's test, (int)d_occlusion[i] < dminl.  d_occlusion / d_filled may be NULL without it. */
int smx_dev_subpixel_pair(int mode, const int64_t* d_keys, const float* d_nbr, const float* d_dmap, const float* d_occlusion,
                          const float* d_filled, int w, int h, int dminl, float* d_sub, float* d_sub_filled, void* stream);
/* delta for one pixel, on the host (no GPU): the formula of smx_dev_subpixel_pair, bit for bit; 0 for a bad mode */
float smx_subpixel_delta(int mode, float c0, float lo, float hi);

/* Synchronous health check of the last smx_dev_aggregate_wta[_pair] call that used d_workspace:
 * copies the call's status word back (call it after synchronising the launch stream).  SMX_E_HIP if
 * a workgroup of the fused kernel gave up waiting for another one (its left neighbour strip or the
 * guidance of its strip; the spins are bounded, 2 s), in which case the results are invalid.  The
 * waits cannot deadlock (every wait is for a work item with a smaller ticket), so this only fires
 * if the GPU is taken away mid-launch; the host-pointer wrappers call it for you. */
int smx_dev_agg_status(const void* d_workspace);
/* Materialised cost volumes (d_cost != NULL) and radius 9: the comb walker loads the costs and checks that each is +0 or a
 * normal number in [2^-60, 2^60] -- what its exactness argument covers (costVolume.cu:187 produces nothing else).  A
 * call with other values (negative, -0, denormal, infinite, NaN) is still answered bit-exactly: the ring walker is queued
 * behind the comb walker and redoes the chunk on the device when the check fired.  This reports, after synchronising the
 * stream, whether that happened in the last call that used d_workspace (the call then cost about 2.5 x). */
int smx_dev_agg_fallback(const void* d_workspace, int* ring_walker_reran);

/* Aggregation implementation of the calling THREAD's smx_dev_* and host-pointer stage calls (a persistent
 * context carries its own, smx_ctx_set_agg_path; it starts with the creating thread's):
 *   0 = auto: the fused single-kernel aggregation when radius <= 9 and -- where the costs are built from the images --
 *       th_color <= 59745 and th_grad <= 59872 (the cost of a partner outside the image comes from a sentinel cell of
 *       60000 that must saturate both truncations), else the multi-kernel path; the fused call picks the comb walker
 *       (smx_agg_v5.hip: radius 9, 1 <= eps < 1e30, costs built from the images, alpha in [0, 1], th_color <= 59744 and
 *       both thresholds exact in fp16) or the ring walker
 *       (smx_agg_v4.hip: any radius <= 9, materialised cost volumes)
 *   1 = force multi-kernel            2 = force fused (error where no walker applies), walker chosen as in auto
 *   3 = fused, ring walker forced     5 = fused, comb walker forced (error where it does not apply)
 *   4 = FAST, NOT bit-exact; reported separately, never a default.  Where the comb walker applies: the same sums in the
 *       same order, window means by multiplication with the rounded reciprocal of the area instead of the exact division
 *       (aggregated costs within ~2.4e-4 relative).  Elsewhere: the ring walker with wave-parallel, re-associated row
 *       prefix sums (within ~4e-3).
 * smx_last_agg_path() reports what the last aggregation on this thread ran: 1 multi-kernel, 2 ring walker,
 * 4 FAST, 5 comb walker. */
int smx_set_agg_path(int path);
int smx_last_agg_path(void);
/* Slices per launch of the fused aggregation.  The reference's slice loop (guidedFilter.cu:171-238) handles ONE slice per
 * iteration; the fused walker handles as many per launch as the caller's workspace holds, and accumulates the running WTA
 * across launches.  smx_set_max_slices_per_launch(n > 0) bounds that number for the calling thread's calls whatever the
 * workspace holds (0 = no bound, the default) -- the knob behind `slices_in_flight` of the Python pipeline and bench.py.
 * It also bounds the chunks in which a context's pair call (smx_ctx_stereo_pair[_rgb]) walks the slices with the census or
 * AD-Census cost, colour guidance or cross-based aggregation on; no chunking changes a bit.
 * smx_last_agg_chunk reports what the calling thread's last fused aggregation did: slices per walker launch (of the first,
 * i.e. largest, launch) and the number of walker launches. */
int smx_set_max_slices_per_launch(int n);
/* d_keys of smx_dev_aggregate_wta[_pair[_cost]] is IN/OUT (shards and chunks accumulate into it; initialise with
 * smx_dev_init_keys).  smx_set_keys_fresh(1) tells the calling thread's following aggregation calls that the keys hold
 * nothing yet: the call's first WTA pass starts from the identity instead of loading them, which saves the
 * smx_dev_init_keys launch (7 us and 7.5 MB of stores per KITTI pair).  smx_set_keys_fresh(0) restores IN/OUT. */
int smx_set_keys_fresh(int on);
int smx_last_agg_chunk(int* slices_per_launch, int* walker_launches);
/* Tile geometry of the fused aggregation for a box radius: output columns per strip, rows per band,
 * columns computed per strip (strip_cols + 2*radius + 1).  For tests that aim at tile boundaries. */
int smx_agg_geometry(int radius, int* strip_cols, int* band_rows, int* tile_cols);

/* winner_take_all.cuh (live WTA = dispSelectOnGPU, guidedFilter.cu:403-411), packed form. */
int smx_dev_init_keys(int64_t* d_keys, int64_t n, void* stream);
/* Fold keys into best/dmap with the reference's rule: if (best >= q) { dmap = dmin + slice;
 * best = q; }.  best/dmap are IN/OUT (use smx_dev_init_wta for the reference's presets). */
int smx_dev_apply_keys(const int64_t* d_keys, int64_t n, int dmin, float* d_best, float* d_dmap,
                       void* stream);
/* main.cu:112-118: best <- 0x7F7F7F7F bit pattern, dmap <- 0. */
int smx_dev_init_wta(float* d_best, float* d_dmap, int64_t n, void* stream);

int smx_dev_filter(const smx_params* p, const uint8_t* d_image, int w, int h, uint8_t* d_mean,
                   float* d_var, void* stream);

int smx_dev_detect_occlusion(const smx_params* p, float* d_dL, const float* d_dR, int dOcclusion,
                             int w, int h, void* stream);
int smx_dev_fill_occlusion(float* d_disp, int w, int h, float vMin, void* stream);
/* main.cu:112-155 behind the aggregation, for both views at once: d_keys / d_best / d_dmap hold the left
 * view in [0, n) and the right one in [n, 2n), n = w*h.  best <- preset, dmap <- 0, the winning slice of
 * every key applied (smx_dev_init_wta + smx_dev_apply_keys), d_occlusion <- left map after the LR check
 * (smx_dev_detect_occlusion with dOcclusion), d_filled <- d_occlusion filled (smx_dev_fill_occlusion with
 * vMin).  One launch (three for rows of more than 8192 pixels) instead of seven; same results (tested against
 * the per-call sequence). */
int smx_dev_finish_pair(const smx_params* p, const int64_t* d_keys, int w, int h, int dminl, int dminr,
                        int dOcclusion, float vMin, float* d_best, float* d_dmap, float* d_occlusion,
                        float* d_filled, void* stream);

/* ------------------------------------------------------------------------------------
 * Weighted-median refinement (not a stage of the reference; opt-in, after fill_occlusion)
 * ---------------------------------------------------------------------------------- */

/* The bilateral weighted median of Hosni et al. (Fast Cost-Volume Filtering, CVPR 2011 / PAMI 2013) that removes the
 * horizontal streaks of the scan-line fill.  Defaults: radius 9, sigma_s 9.0, sigma_c 25.5 (0.1 on a [0, 1] intensity
 * scale).  Valid: 1 <= radius <= 15, sigma_s and sigma_c finite and > 0. */
typedef struct smx_wmf_params {
    int radius;       /* window (2*radius+1)^2, clipped to the image (no padding) */
    double sigma_s;   /* spatial */
    double sigma_c;   /* range (gray levels) */
} smx_wmf_params;
void smx_default_wmf_params(smx_wmf_params* p);

/* The integer weight tables, computed on the host in double (works without a GPU):
 *   spatial[k] = floor(1023 * exp(-k / sigma_s^2) + 0.5)   k = dx^2 + dy^2 = 0 .. 2*radius^2
 *   range[t]   = floor(1023 * exp(-t^2 / sigma_c^2) + 0.5) t = |guide(p) - guide(q)| = 0 .. 255
 * The weight of sample q for output pixel p is w(p, q) = spatial[dx^2 + dy^2] * range[t] (< 2^20), so a window's sum
 * is below 2^30 and every sum is exact in any order. */
int smx_wmf_weights(const smx_wmf_params* p, uint16_t* spatial, uint16_t* range);

/* out = weighted median of disp guided by `guide` (u8 gray of the view the map belongs to), labels [dmin, dmin+size_d).
 *   samples:  the pixels q of the window centred on p, clipped to the image; q counts only if disp[q] is an integer in
 *             [dmin, dmin + size_d) (-0.0 is the integer 0; NaN, +-inf, fractions, labels out of range and the LR-check
 *             marker dmin - 100 count for nothing)
 *   result:   (float)(dmin + k*), k* the SMALLEST k with 2 * cum(k) >= total, where total = sum of the weights of the
 *             counting samples and cum(k) = the sum over those with label <= dmin + k; if total == 0, disp[p]
 *   select:   NULL filters every pixel; otherwise pixel i is filtered iff (int)select[i] < dmin (select[i] truncated
 *             toward zero; NaN and +-inf select nothing) -- fill_occlusion's test, so passing the pair's occlusion map
 *             filters exactly the pixels the LR check invalidated.  Pixels that are not filtered are copied bit for bit.
 * out must not be disp (SMX_E_ARG).  1 <= size_d <= 4096, dmin + size_d <= INT_MAX; any width (rows are not staged whole).
 * smx_weighted_median: host pointers, synchronous.  smx_dev_weighted_median: device pointers, one kernel launch on
 * `stream`, no allocation, no synchronisation, no workspace (graph-capturable). */
int smx_weighted_median(const smx_wmf_params* p, const uint8_t* guide, const float* disp, const float* select,
                        float* out, int w, int h, int dmin, int size_d);
int smx_dev_weighted_median(const smx_wmf_params* p, const uint8_t* d_guide, const float* d_disp,
                            const float* d_select, float* d_out, int w, int h, int dmin, int size_d, void* stream);

/* ------------------------------------------------------------------------------------
 * Census / Hamming matching cost (not a stage of the reference; opt-in alternative to compute_cost)
 * ---------------------------------------------------------------------------------- */

/* The census transform (Zabih & Woodfill) with a Hamming-distance cost.  It depends only on the ORDER of the gray values
 * in a window, so a strictly increasing change of one image's intensities (exposure, gain) leaves the volume untouched.
 * Defaults: rx 4, ry 3 (a 9 x 7 window, 62 bits), th 62.  Valid: 1 <= rx <= 4, 1 <= ry <= 3, th >= 1.
 *   code  of pixel (y, x) of image I: a uint64_t.  The window's neighbours are numbered k = 0, 1, ... with dy = -ry .. ry in
 *         the outer loop and dx = -rx .. rx in the inner one, the centre skipped; bit k (bit 0 = LSB) is set iff
 *         I[clamp(y + dy, 0, h - 1)][clamp(x + dx, 0, w - 1)] < I[y][x].  (Replicate clamp: an image smaller than the
 *         window is legal.)  nbits = (2 rx + 1)(2 ry + 1) - 1 <= 62.
 *   cost  of view v, slice z: own = the view's codes, other = the other view's, d = dmin_v + z, t = min(th, nbits):
 *         cost[z][y][x] = (float)min(popcount(own[y][x] ^ other[y][x + d]), t) if 0 <= x + d < w, else (float)t.
 *         Layout [z][y][x], slice z at (z - s_begin) * w*h, xx = x + d: as smx_dev_cost_volume.
 * The costs are small non-negative integers: every aggregation path takes them as materialised volumes
 * (smx_dev_aggregate_wta_pair_cost, the _nbr forms), the comb walker without its fall-back. */
typedef struct smx_census_params {
    int rx, ry;   /* window (2 rx + 1) x (2 ry + 1) */
    int th;       /* truncation of the Hamming distance; the cost of a partner outside the image */
} smx_census_params;
void smx_default_census_params(smx_census_params* p);
/* (2 rx + 1)(2 ry + 1) - 1, or SMX_E_ARG for invalid parameters.  Host only, no GPU. */
int smx_census_bits(const smx_census_params* p);

/* d_img: nimages contiguous w*h u8 planes -> d_code: nimages contiguous w*h planes of codes, one launch (a pair passes 2). */
int smx_dev_census(const smx_census_params* p, const uint8_t* d_img, uint64_t* d_code, int w, int h, int nimages,
                   void* stream);
/* d_code: the codes of the left image, then those of the right one (2 * w*h).  Slices [s_begin, s_end) of the left volume
 * (labels dminl + z) into d_cost_l and of the right volume (labels dminr + z) into d_cost_r, both in one launch; either
 * cost pointer may be NULL (not both), which gives the single-view form.  w, h >= 1. */
int smx_dev_census_cost_pair(const smx_census_params* p, const uint64_t* d_code, float* d_cost_l, float* d_cost_r, int w,
                             int h, int dminl, int dminr, int s_begin, int s_end, void* stream);
/* Host pointers, synchronous; mirrors smx_compute_cost: the volume of i1 against i2, size_d*w*h floats, labels dmin + z. */
int smx_census_cost(const smx_census_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h,
                    int size_d, int dmin);

#define SMX_COST_REFERENCE 0   /* compute_cost (costVolume.cu): the default */
#define SMX_COST_CENSUS 1
/* Matching cost of this context.  With SMX_COST_CENSUS (census: NULL = the defaults) smx_ctx_stereo_pair builds the codes
 * once per pair, then runs census cost chunk -> aggregation from that chunk (the _pair_cost form, or _pair_nbr with
 * sub-pixel on) over ascending contiguous chunks of slices, then the usual finish; cost_l / cost_r of smx_pair_out receive
 * the census volumes; th_color / th_grad / alpha of smx_params are unused, radius, eps and d_lr apply as always.  The code
 * and chunk buffers are allocated on first use.  smx_ctx_stereo_pair_async returns SMX_E_ARG while census is on. */
int smx_ctx_set_cost(smx_ctx* ctx, int mode, const smx_census_params* census);

/* ------------------------------------------------------------------------------------
 * Speckle removal (not a stage of the reference; opt-in, between the LR check and fill_occlusion)
 * ---------------------------------------------------------------------------------- */

/* OpenCV's filterSpeckles rule: small islands of mutually consistent disparity are invalidated, so that the scan-line
 * fill (and wmf "occluded") replaces them.  Defaults: max_size 200, max_diff 1.0f.
 *   counts:   a pixel p counts iff disp[p] is finite and passes fill_occlusion's validity test against vmin, i.e.
 *             (float)(int)disp[p] >= vmin with the truncation toward zero (saturating at +-2^31) and the comparison of
 *             k_fill_occlusion.  NaN and +-inf never count; -0.0 is 0; the LR-check marker dmin - 100 does not count
 *             (with vmin = dmin).
 *   joined:   4-neighbours p, q are joined iff both count and fabsf(disp[p] - disp[q]) <= max_diff, evaluated in f32
 *             without contraction (numpy float32 gives the same bits), fractional (sub-pixel) maps included.
 *   components: the connected components of that graph (the relation is not transitive; the components are well
 *             defined: a chain a, a + 1, a + 2 is one component at max_diff 1).
 *   result:   out[p] = new_val iff p counts and its component has <= max_size pixels; every other pixel is copied bit
 *             for bit.  max_size == 0 copies the map.
 * d_out == d_disp is allowed.  Valid: max_size >= 0, max_diff finite and >= 0, w, h >= 1, w*h < 2^31 (SMX_E_ARG
 * otherwise); a workspace smaller than smx_speckle_workspace_bytes(w, h) is SMX_E_WS (about 8 bytes per pixel: a u32
 * label plane and a u32 size plane; 0 for invalid w, h).  The workspace needs no alignment and may hold anything.
 * smx_dev_speckle_filter: device pointers, four kernel launches on `stream`, no allocation, no synchronisation
 * (graph-capturable); it touches only [0, smx_speckle_workspace_bytes) of d_ws and the w*h floats of d_out.  The result
 * does not depend on scheduling: it is the same bits in every run.
 * smx_speckle_filter: host pointers, synchronous. */
typedef struct smx_speckle_params {
    int max_size;     /* components of at most this many pixels are invalidated */
    float max_diff;   /* largest difference between joined 4-neighbours */
} smx_speckle_params;
void smx_default_speckle_params(smx_speckle_params* p);
size_t smx_speckle_workspace_bytes(int w, int h);
int smx_dev_speckle_filter(const smx_speckle_params* p, const float* d_disp, float* d_out, int w, int h, float vmin,
                           float new_val, void* d_ws, size_t ws_bytes, void* stream);
int smx_speckle_filter(const smx_speckle_params* p, const float* disp, float* out, int w, int h, float vmin,
                       float new_val);
/* Test hook, NOT part of the stable contract (it may change or go with the kernels): the tile of the labelling kernel
 * (columns, rows), so that the tests put their shapes and components on the seams between tiles. */
int smx_speckle_geometry(int* tile_cols, int* tile_rows);
/* Speckle removal of this context: NULL switches it off (the default).  While it is on, smx_ctx_stereo_pair filters the
 * left map after the LR check with vmin = dminl, new_val = dminl - 100; out->filled is the fill of the despeckled map and
 * the sub-pixel fit's sub_filled takes the despeckled map for its test; out->occlusion stays the LR-check map.
 * smx_ctx_stereo_pair_async returns SMX_E_ARG.  smx_ctx_speckle_map copies the despeckled map of the last synchronous
 * smx_ctx_stereo_pair of the context (n floats); SMX_E_ARG if that pair ran without it.  Buffers are allocated on first use. */
int smx_ctx_set_speckle(smx_ctx* ctx, const smx_speckle_params* p);
int smx_ctx_speckle_map(smx_ctx* ctx, float* despeckled);

/* ------------------------------------------------------------------------------------
 * Semi-global matching (not a stage of the reference; opt-in alternative to the guided-filter aggregation)
 * ---------------------------------------------------------------------------------- */

/* SGM (Hirschmueller 2008) with constant penalties over whole cost volumes.  Defaults: p1 10, p2 120, paths 8 (libSGM's for
 * a census cost of this size).  Valid: 0 <= p1 <= p2 <= 4095, paths 4 or 8; w, h >= 1, w*h < 2^31,
 * 1 <= size_d <= SMX_SGM_MAX_D (SMX_E_ARG otherwise).
 *   input:      one cost volume per view, f32, [z][y][x] (smx_dev_census_cost_pair, smx_dev_cost_volume).  Each value is
 *               read as the integer C = c >= 0 ? (c <= 255 ? (int)c : 255) : 0, so NaN gives 0: the call is total, memory-
 *               safe and deterministic on any bits.
 *   directions: (dx, dy) = (1,0) (-1,0) (0,1) (0,-1) for paths 4; also (1,1) (-1,1) (1,-1) (-1,-1) for paths 8.
 *   recurrence: for a direction r and a pixel p: L_r(p, d) = C(p, d) if p - r lies outside the image; otherwise, with
 *               m = min_k L_r(p - r, k),
 *                 L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + p1, L_r(p-r, d+1) + p1, m + p2) - m
 *               where terms with d-1 < 0 or d+1 >= size_d are left out.  Integers throughout: L_r <= 255 + p2 <= 4350 and
 *               S(p, d) = sum_r L_r(p, d) <= 34800, exact in u16 and in f32 in any order, so the result is the same bits
 *               in every run whatever the schedule.
 *   d_keys:     OUT only: d_keys[p] = smx_pack_key((float)S(p, z*), z*), z* the LARGEST z of minimal S (the project's tie
 *               rule: the last slice of equal costs wins) -- the keys of a fresh winner-take-all over the f32 volume S.
 *   d_agg:      optional, size_d * n floats: (float)S in [z][y][x].
 *   d_nbr:      optional, 3n floats in the layout and meaning of the _nbr state after one whole-volume call:
 *               lo = S(z* - 1) (NaN at z* = 0), hi = S(z* + 1) (NaN at z* = size_d - 1), last = S(size_d - 1);
 *               smx_dev_subpixel_pair works on it unchanged.
 * SGM needs the whole disparity range of a pixel at once: there is no s_begin / s_end, no accumulation into existing keys
 * and no combination across D-shards.
 * smx_dev_sgm_wta_pair: either cost pointer may be NULL (not both), the one-view form, whose outputs hold that one view;
 * with both, d_keys holds 2n keys, d_agg two volumes and d_nbr 6n floats, left view first.  A fixed sequence of kernel
 * launches on `stream` (5 for paths 4, 9 for paths 8), no allocation, no synchronisation (graph-capturable).  d_ws needs no
 * alignment and may hold anything; fewer than smx_sgm_workspace_bytes(w, h, size_d, nviews) bytes is SMX_E_WS before
 * anything is launched (about 3 bytes per pixel and disparity, size_d rounded up to 64; 0 for invalid sizes or nviews
 * other than 1, 2).  Nothing is written outside the workspace and the stated extents; the inputs are not modified.
 * smx_sgm_aggregate: host pointers, synchronous, one view.  agg (optional) receives S; best (optional, n floats) the
 * winner's S and disp_map (optional, n floats) dmin + z*, both OUT only. */
#define SMX_SGM_MAX_D 256
typedef struct smx_sgm_params { int p1, p2; int paths; } smx_sgm_params;
void smx_default_sgm_params(smx_sgm_params* p);
size_t smx_sgm_workspace_bytes(int w, int h, int size_d, int nviews);
int smx_dev_sgm_wta_pair(const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                         int64_t* d_keys, float* d_agg, float* d_nbr, void* d_ws, size_t ws_bytes, void* stream);
int smx_sgm_aggregate(const smx_sgm_params* p, const float* cost, float* agg, float* best, float* disp_map, int w, int h,
                      int size_d, int dmin);

#define SMX_AGG_GUIDED 0   /* the reference's guided filter: the default */
#define SMX_AGG_SGM 1
/* Aggregation of this context.  With SMX_AGG_SGM (sgm: NULL = the defaults) smx_ctx_stereo_pair builds both whole cost
 * volumes (census, or the reference cost read through the clamp above), runs smx_dev_sgm_wta_pair (with the neighbour state
 * when sub-pixel is on), then the usual finish, speckle removal and sub-pixel fit.  agg_l / agg_r of smx_pair_out receive S;
 * mean_l / mean_r are not produced (SMX_E_ARG if requested); radius and eps of smx_params are unused.  The volumes and the
 * workspace are allocated on first use.  smx_ctx_stereo_pair_async returns SMX_E_ARG while it is on. */
int smx_ctx_set_aggregation(smx_ctx* ctx, int mode, const smx_sgm_params* sgm);

/* ------------------------------------------------------------------------------------
 * Hierarchical belief propagation (not a stage of the reference; opt-in alternative to the guided-filter aggregation)
 * ---------------------------------------------------------------------------------- */

/* Min-sum loopy belief propagation on the 4-connected pixel grid with a truncated-linear smoothness term, after Felzenszwalb
 * and Huttenlocher, "Efficient Belief Propagation for Early Vision" (IJCV 2006): O(D) messages, a checkerboard schedule that
 * updates in place, a coarse-to-fine pyramid.  Integers throughout, so the result is the same bits in every run.
 *   parameters: step 20, trunc 60, iterations 5, levels 4, data_scale 1.0f by default (chosen on synthetic scenes, not measured
 *               on real data).  Valid: 0 <= step <= 4095, 0 <= trunc <= 4095, 0 <= iterations <= 64, 1 <= levels <= 8,
 *               data_scale finite and > 0; w, h >= 1, w*h < 2^31, 1 <= size_d <= SMX_BP_MAX_D.  Anything else is SMX_E_ARG
 *               before any device call.
 *   data term:  one f32 cost volume per view, [z][y][x].  t = c * data_scale is one f32 product and
 *               C = t >= 0 ? (t <= 255 ? (int)t : 255) : 0, so a NaN gives 0: the call is total on any bits.  Level 0 is the
 *               image with D_0 = C.  Level l+1 has size (ceil(w_l / 2), ceil(h_l / 2)); its data term is the sum of the up to
 *               four children (2x .. 2x+1, 2y .. 2y+1) that exist.  D_l <= 255 * 4^l.
 *   smoothness: V(z, z') = min(step * |z - z'|, trunc).
 *   messages:   every pixel p of a level holds four incoming messages, from its left, right, upper and lower neighbour.  A
 *               message from outside the image is 0 and is never updated.  One update of the message q -> p, p a neighbour of q:
 *                 h(z)  = D_l(q, z) + sum of m_{r->q}(z) over the neighbours r of q other than p
 *                 m'(z) = min over z' of (h(z') + V(z, z'))
 *                 m_{q->p}(z) = m'(z) - min_k m'(k)
 *               hence 0 <= m <= trunc, exact in u16; h <= 255 * 4^l + 3 * trunc and every intermediate fits i32.
 *   schedule:   at the coarsest level all messages start at 0.  At every level run iterations t = 1 .. iterations; iteration t
 *               replaces exactly the messages INTO the pixels with (x + y + t) even, each computed from the current messages
 *               into its neighbours (all of the other parity and untouched in that iteration, so the order does not matter).
 *               Going from level l+1 to l, pixel (x, y) takes all four messages of (x >> 1, y >> 1).  With iterations == 0, or
 *               step == trunc == 0, all messages are 0.
 *   belief:     S(p, z) = D_0(p, z) + the four incoming messages at level 0; S <= 255 + 4 * 4095 = 16635, exact in u16 and f32.
 *   outputs:    d_keys, d_agg, d_nbr and d_uq carry, word for word, the meanings they have for smx_dev_sgm_wta_pair(_uq) with
 *               this S: keys are OUT only and the largest z of minimal S wins; d_agg is (float)S in [z][y][x]; d_nbr holds
 *               lo / hi / last with NaN at the ends; d_uq is the state of one run over the whole range.  As for SGM there is no
 *               s_begin / s_end, no accumulation into existing keys and no combination across D-shards.
 * smx_dev_bp_wta_pair: either cost pointer may be NULL (not both), the one-view form, whose outputs are laid out as SGM's;
 * d_agg, d_nbr and d_uq are optional.  A fixed sequence of kernel launches on `stream`, a function of levels and iterations
 * only (4 + 2 * (levels - 1) + levels * iterations), no allocation, no synchronisation (graph-capturable).  d_ws needs no
 * alignment and may hold anything; fewer than smx_bp_workspace_bytes(w, h, size_d, levels, nviews) bytes is SMX_E_WS before
 * anything is launched.  With Dp = size_d rounded up to 64, n_l = w_l * h_l and A(b) = b rounded up to 256 that is
 *   255 + nviews * (A(2 * n_0 * Dp) + sum over l < levels of (A((l ? 4 : 1) * n_l * Dp) + A(8 * n_l * Dp)))
 * bytes: the u16 belief, and per level the data term (u8 at level 0, u32 above) and four u16 message planes -- about 11 bytes
 * per pixel and label at level 0 and a third of 12 more for the coarse levels; 0 for invalid sizes, levels outside 1 .. 8 or
 * nviews other than 1, 2.  Nothing is written outside the workspace and the stated extents; the inputs are not modified.
 * smx_bp_aggregate: host pointers, synchronous, one view; agg, best, disp_map as for smx_sgm_aggregate. */
#define SMX_BP_MAX_D 256
typedef struct smx_bp_params { int step, trunc; int iterations; int levels; float data_scale; } smx_bp_params;
void smx_default_bp_params(smx_bp_params* p);
size_t smx_bp_workspace_bytes(int w, int h, int size_d, int levels, int nviews);
int smx_dev_bp_wta_pair(const smx_bp_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                        int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_bp_aggregate(const smx_bp_params* p, const float* cost, float* agg, float* best, float* disp_map, int w, int h,
                     int size_d, int dmin);
/* Belief propagation as the aggregation of this context (p: the parameters; NULL = off, the default).  The flow of SMX_AGG_SGM:
 * smx_ctx_stereo_pair builds both whole cost volumes (the reference's, census or AD-Census), runs one smx_dev_bp_wta_pair (with
 * the neighbour and uniqueness states when sub-pixel and uniqueness are on), then the unchanged finish: LR check, uniqueness,
 * speckle, vote, fill, adjustment on agg_l, sub-pixel.  agg_l / agg_r of smx_pair_out receive S; radius and eps of smx_params
 * are unused.  The pair call returns SMX_E_ARG with a message together with SMX_AGG_SGM, cross-based aggregation, the
 * scan-line optimiser, colour guidance, cross-scale aggregation, the permeability filter or PatchMatch, when mean_l / mean_r
 * are requested, and with more than SMX_BP_MAX_D labels; smx_ctx_stereo_pair_async returns SMX_E_ARG while it is on.  The
 * workspace is allocated on the first pair that runs with it on: a context that never does holds and launches nothing new.
 * smx_ctx_bp_held (a test hook): the bytes of that workspace, 0 before. */
int smx_ctx_set_bp(smx_ctx* ctx, const smx_bp_params* p);
int smx_ctx_bp_held(const smx_ctx* ctx, size_t* bytes);

/* ------------------------------------------------------------------------------------
 * Uniqueness (peak-ratio) filtering (not a stage of the reference; opt-in, between the LR check and speckle removal)
 * ---------------------------------------------------------------------------------- */

/* The test of OpenCV's uniquenessRatio / libSGM's uniqueness: a winner is ambiguous when a disparity that is not its
 * neighbour costs almost as little.  The aggregated volume q is normally never materialised, so the second-best cost is
 * kept by the one pass that reads every q: the winner-take-all pass.
 *
 * The second-best cost.  For a pixel of one view the slices z come in ascending order with aggregated costs q(z).
 *   winner:  (c0, z*) exactly as in the plain calls: the smallest cost, the last slice among equal costs, a NaN never wins.
 *   sec   =  min { q(k) : k seen, |k - z*| >= 2, q(k) not NaN }, +inf if there is no such slice.  The winner's two
 *            neighbours are left out because a good peak is wide; a tie two or more slices away gives sec == c0.  Among
 *            equal values (-0 == +0) the bits are those of the first such slice.
 * The streaming form.  State per pixel: the key (m, z*), sec, rest = the min of the costs of all seen slices except the last
 * seen (+inf if none), last = the cost of the last seen slice (NaN if none).  At slice z with cost v, in f32 with plain
 * comparisons (a NaN compares false):
 *     take = v <= m
 *     sec  = take ? rest : ((z >= z* + 2 && v < sec) ? v : sec)
 *     m, z* = take ? (v, z) : (m, z*)
 *     rest = last < rest ? last : rest ;  last = v
 * When the winner moves to z, everything up to z - 2 is non-adjacent to it: that is `rest`.  A run resumed from the stored
 * state (m, z* unpacked from the key; an identity key starts blank and reads no state) equals one run over all slices,
 * whatever the chunking; there is no merge step.
 *
 * State.  d_uq holds three f32 planes [3][h][w] per view: 0 sec, 1 rest, 2 last (6n floats for a pair, left view first).
 *   - IN/OUT like d_keys; it needs no initialisation: a pixel whose key is the identity, or a call made with fresh keys
 *     (smx_set_keys_fresh), starts without state.
 *   - Calls on one set of keys must cover ascending, contiguous slice ranges (the _nbr rule).
 *   - It does not combine across D-shards, and it is independent of d_nbr: both may be requested in one call.
 *
 * smx_dev_aggregate_wta_pair_uq: smx_dev_aggregate_wta_pair_nbr that also keeps d_uq (required); d_nbr NULL or 6n floats;
 * d_cost_l / d_cost_r both NULL or both set.  Keys (and d_nbr, d_agg, d_mean_u8) are those of the other entries, bit for
 * bit.  It honours smx_set_max_slices_per_launch, smx_set_keys_fresh, every aggregation path and the queued ring-walker
 * fall-back; same workspace, same number of launches.
 * smx_dev_sgm_wta_pair_uq: smx_dev_sgm_wta_pair that also writes d_uq (required; 3n floats per view of the call) after its one
 * run over the whole range; same launches, same workspace.  Exact: S are integers. */
int smx_dev_aggregate_wta_pair_uq(const smx_params* p, const uint8_t* d_left, const uint8_t* d_right,
                                  const float* d_cost_l, const float* d_cost_r, int w, int h, int dminl, int dminr,
                                  int s_begin, int s_end, int64_t* d_keys, uint8_t* d_mean_u8, float* d_agg,
                                  void* d_workspace, size_t workspace_bytes, float* d_nbr, float* d_uq, void* stream);
int smx_dev_sgm_wta_pair_uq(const smx_sgm_params* p, const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d,
                            int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes,
                            void* stream);
/* The test, one view: c0 = the cost of d_keys[p], s = d_uq[p] (the sec plane; n = w*h keys and floats are read).
 *   rejected: pixel p is rejected iff its key is not the identity, ratio > 0 and s - c0 < ratio * fabsf(c0), in f32 without
 *             contraction.  ratio: finite and >= 0 (SMX_E_ARG otherwise); 0 rejects nothing; OpenCV's u percent is
 *             ratio = u / (100 - u).  An unknown s (+inf, NaN) is never rejected.
 *   result:   d_out[p] = new_val iff d_disp[p] counts -- the speckle filter's validity rule against vmin -- and p is
 *             rejected; every other pixel is copied bit for bit.  d_out == d_disp is allowed.
 *   d_margin: NULL, or n floats out: s - c0, +inf where s is unknown, NaN where the key is the identity.
 * smx_dev_uniqueness: device pointers, one kernel launch on `stream`, no allocation, no synchronisation, no workspace
 * (graph-capturable); it writes the n floats of d_out and of d_margin only.  smx_uniqueness_filter: host pointers,
 * synchronous; uq needs its first n floats (the sec plane) only. */
int smx_dev_uniqueness(float ratio, const int64_t* d_keys, const float* d_uq, const float* d_disp, float* d_out,
                       float* d_margin, int w, int h, float vmin, float new_val, void* stream);
int smx_uniqueness_filter(float ratio, const int64_t* keys, const float* uq, const float* disp, float* out, float* margin, int w,
                          int h, float vmin, float new_val);
/* The uniqueness test of this context: ratio 0 switches it off (the default); NaN, negative or infinite is SMX_E_ARG.  While
 * it is on, smx_ctx_stereo_pair keeps the state of both views (with either cost, either aggregation and both census chunk
 * loops) and filters the left map after the LR check with vmin = dminl, new_val = dminl - 100.  Order: LR check -> uniqueness
 * -> speckle -> fill -> sub-pixel sub_filled; out->filled is the fill of the last of these maps, out->occlusion stays the
 * LR-check map.  smx_ctx_stereo_pair_async returns SMX_E_ARG.  smx_ctx_uniqueness_map copies the filtered map and the
 * margins of the last synchronous smx_ctx_stereo_pair of the context (n floats each; either may be NULL); SMX_E_ARG if that
 * pair ran without the test.  Buffers are allocated on first use. */
int smx_ctx_set_uniqueness(smx_ctx* ctx, float ratio);
int smx_ctx_uniqueness_map(smx_ctx* ctx, float* map, float* margin);

/* ------------------------------------------------------------------------------------
 * Colour (RGB) guidance for the guided-filter aggregation (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The guided filter of He et al. with a colour guide, as in Hosni / Rhemann et al.'s cost-volume filtering: the 3 x 3
 * covariance of the guide per window instead of the gray variance, so that an edge between two colours of equal luminance
 * stays an edge.  tests/cgf_ref.py is this definition in numpy; the result equals it bit for bit.
 *   inputs:    per view the guide, u8 [h][w][channels], channels 3 or 4 with R, G, B the first three bytes, and the cost
 *              volume, materialised: f32 [z][y][x], slice s of [s_begin, s_end) at d_cost[(s - s_begin) * w*h].
 *   integral:  f32, row prefix left to right, then column prefix top to bottom, each a sequential chain acc = v + acc from
 *              -0.0f (integral.cu:78-131, as everywhere in this library).
 *   box mean:  the clamped window of radius `radius`: ((S11 - S10) - S01) + S00 with the taps outside the image left out,
 *              divided by (float)area (computeMeanOnGPU guidedFilter.cu:305-318).
 *   guidance, once per view: I_c = (float)u8 for c in r, g, b; the six products I_c I_c' (exact in f32); the nine box means
 *              mu_c, m_cc'; v_cc' = m_cc' - mu_c * mu_c' (the product rounded before the difference).  Then in double, every
 *              product and every sum rounded on its own:
 *                a = (double)v_rr + eps, b = v_rg, c = v_rb, d = v_gg + eps, e = v_gb, f = v_bb + eps
 *                A = d*f - e*e, B = c*e - b*f, C = b*e - c*d, D = a*f - c*c, E = b*c - a*e, F = a*d - b*b
 *                det = (a*A + b*B) + c*C
 *              and six f32 planes (float)(X / det), X = A .. F: the rows (A B C; B D E; C E F) of (Sigma + eps I)^-1.  A zero
 *              or negative det gets no special treatment: what IEEE gives propagates, and a NaN never wins.
 *   per slice p: box means mu_p and m_cp of p and of I_c * p (f32 product); cov_c = m_cp - mu_c * mu_p;
 *                a_r = (A cov_r + B cov_g) + C cov_b, a_g = (B cov_r + D cov_g) + E cov_b, a_b = (C cov_r + E cov_g) + F cov_b;
 *                b = mu_p - ((a_r mu_r + a_g mu_g) + a_b mu_b); box means of a_r, a_g, a_b, b give abar_c, bbar;
 *                q = ((abar_r I_r + abar_g I_g) + abar_b I_b) + bbar.  All f32, left to right.
 *   winner:    the packed keys and the tie rule of smx_dev_aggregate_wta (the last slice of equal costs wins).
 *   parameters: radius (any >= 0) and eps of smx_params; nothing else of it is read.
 *
 * smx_dev_cgf_wta_pair: both views in every launch.  Either rgb / cost pair may be NULL (not both; a view's guide and cost
 * come together) for the one-view form, whose outputs hold that one view.
 *   d_keys:  IN/OUT like smx_dev_aggregate_wta_pair_cost: n keys per view (left first), accumulated across calls and across
 *            D-shards by the int64 min; smx_set_keys_fresh does not apply: the keys are always loaded.
 *   d_agg:   optional, (s_end - s_begin) * n floats per view: q.
 *   d_nbr, d_uq: optional, 3n floats per view each: the neighbour state and the second-best state of the _nbr / _uq entries
 *            above, with their meaning and their rule (ascending, contiguous ranges on one set of keys).
 * The slices go in chunks that fit the workspace (smx_set_max_slices_per_launch bounds the chunk as well); the chunking does
 * not change a bit.  Per chunk six kernel launches, four more per call for the guidance; no allocation, no synchronisation
 * (graph-capturable).  smx_cgf_workspace_bytes(w, h, nslices, nviews) holds `nslices` slices in flight: per view 9 guidance
 * planes and max(9, 8 * nslices) working planes of w*h floats, plus 255 bytes (0 for invalid sizes: w, h >= 1, h <= 65535,
 * w*h < 2^31, nslices >= 1, nviews 1 or 2).  Fewer bytes than for one slice is SMX_E_WS before anything is launched.  The
 * memory contract is that of the aggregation entries above smx_agg_workspace_bytes: nothing is written outside the workspace
 * and the stated extents, the workspace may hold anything and needs no alignment, the inputs are not modified.
 * smx_colour_guided_filter: host pointers, one view, synchronous; filter_cost / disp_map IN/OUT and agg as for
 * smx_compute_guided_filter (there is no mean image). */
size_t smx_cgf_workspace_bytes(int w, int h, int nslices, int nviews);
int smx_dev_cgf_wta_pair(const smx_params* p, const uint8_t* d_rgb_l, const uint8_t* d_rgb_r, int channels,
                         const float* d_cost_l, const float* d_cost_r, int w, int h, int s_begin, int s_end, int64_t* d_keys,
                         float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_colour_guided_filter(const smx_params* p, const uint8_t* rgb, int channels, const float* cost, float* filter_cost,
                             float* disp_map, float* agg, int w, int h, int size_d, int dmin);

#define SMX_GUIDE_GRAY 0   /* the reference's gray guide: the default */
#define SMX_GUIDE_RGB 1
/* Guidance of this context's guided filter.  smx_ctx_stereo_pair_rgb takes the pair as colour images (u8 [h][w][channels],
 * channels 3 or 4), makes the gray images on the device (smx_dev_rgb_to_grayscale) for the matching cost -- the reference's,
 * or census per smx_ctx_set_cost -- and then runs the pair as smx_ctx_stereo_pair does: with SMX_GUIDE_GRAY it equals
 * smx_ctx_stereo_pair on the converted images; with SMX_GUIDE_RGB both cost volumes go chunk by chunk through
 * smx_dev_cgf_wta_pair (with the neighbour and second-best states where sub-pixel or uniqueness are on), then the usual finish,
 * uniqueness, speckle removal and sub-pixel fit.  cost_* / agg_* of smx_pair_out receive the volumes.  The colour images, the
 * workspace and the chunk buffers are allocated on first use.  While SMX_GUIDE_RGB is on: mean_l / mean_r are not produced
 * (SMX_E_ARG if requested); SMX_AGG_SGM is SMX_E_ARG at the pair call; smx_ctx_stereo_pair, which has no colour images, and
 * smx_ctx_stereo_pair_async return SMX_E_ARG. */
int smx_ctx_set_guidance(smx_ctx* ctx, int mode);
int smx_ctx_stereo_pair_rgb(smx_ctx* ctx, const uint8_t* rgb_l, const uint8_t* rgb_r, int channels, int dminl, int dminr,
                            const smx_pair_out* out);

/* ------------------------------------------------------------------------------------
 * AD-Census matching cost: census plus absolute differences (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The census cost throws away everything but the ORDER of the gray values in its window: two patches of equal local order and
 * different magnitudes cost 0 against each other (a periodic pattern whose periods differ in brightness ties between the true
 * label and the labels one period away).  AD-Census (Mei et al. 2011) adds the absolute difference of the pixels, each term
 * through rho(c, lambda) = 1 - exp(-c / lambda): the term that discriminates dominates and neither runs away.
 * tests/adcensus_ref.py is this definition in numpy; the volume equals it bit for bit.
 * Defaults: the census defaults, lambda_census 30, lambda_ad 10, scale 127.5, colour 0.  Valid: the census part as for
 * smx_census_bits; both lambda finite with 0 < lambda <= 1e6; scale finite with 2^-20 <= scale <= 2^20; colour 0 or 1.
 *   tables, computed on the host in double (nch = 3 if colour else 1), SMX_ADCENSUS_TABLE_FLOATS floats:
 *         T[k]      = (float)(scale * (1.0 - exp(-(double)k / lambda_census)))          k = 0 .. 63
 *         T[64 + s] = (float)(scale * (1.0 - exp(-(double)s / ((double)nch * lambda_ad))))   s = 0 .. 765
 *         T[0] and T[64] are +0.0 and every other entry is a normal number in [2^-60, 2^60]: the value set of the comb
 *         walker's exactness argument (smx_dev_agg_fallback), so no aggregation path takes its fall-back.  With the default
 *         scale the cost lies in [0, 255], which the clamp of smx_dev_sgm_wta_pair keeps.
 *   cost  of view v, slice z: own = the view, other = the other one, d = dmin_v + z, xx = x + d, t = min(th, nbits), the
 *         codes those of smx_dev_census on the gray images.  If 0 <= xx < w:
 *           hc = min(popcount(code_own[y][x] ^ code_other[y][xx]), t)
 *           s  = sum over the channels c of |own_c[y][x] - other_c[y][xx]|    (one gray channel, or R, G, B: the first three
 *                bytes of a pixel; a 4th byte is ignored)
 *           cost[z][y][x] = T[hc] + T[64 + s]                                  (one f32 addition)
 *         else cost[z][y][x] = T[t] + T[64 + 255 * nch].
 *         Layout, slice placement and [s_begin, s_end) as for smx_dev_census_cost_pair. */
typedef struct smx_adcensus_params {
    smx_census_params census;   /* window and Hamming truncation, as for the census cost */
    double lambda_census;       /* default 30 */
    double lambda_ad;           /* default 10 */
    double scale;               /* default 127.5: the cost lies in [0, 255], which SGM's clamp keeps */
    int colour;                 /* 0: AD on the gray images; 1: AD on R, G, B of the colour images */
} smx_adcensus_params;
#define SMX_ADCENSUS_TABLE_FLOATS (64 + 766)
void smx_default_adcensus_params(smx_adcensus_params* p);
/* The tables above into `tables` (SMX_ADCENSUS_TABLE_FLOATS floats).  Host only: works without a GPU. */
int smx_adcensus_tables(const smx_adcensus_params* p, float* tables);
/* The same into device memory: a set-up call that copies from host memory and waits for the copy on `stream`.  NOT
 * graph-capturable: upload the table once, outside any capture. */
int smx_dev_adcensus_tables(const smx_adcensus_params* p, float* d_tables, void* stream);
/* d_tables: smx_dev_adcensus_tables of the same parameters; d_code: the codes of the left gray image, then those of the right
 * one (smx_dev_census with p->census); d_img_l / d_img_r: u8 [h][w][channels], channels 1 with colour 0 (the gray images), 3 or
 * 4 with colour 1 (anything else is SMX_E_ARG).  Slices [s_begin, s_end) of the left volume (labels dminl + z) into d_cost_l
 * and of the right volume (labels dminr + z) into d_cost_r, both in one launch; either cost pointer may be NULL (not both),
 * which gives the single-view form.  One launch, no allocation, no synchronisation (graph-capturable).  w, h >= 1. */
int smx_dev_adcensus_cost_pair(const smx_adcensus_params* p, const float* d_tables, const uint64_t* d_code,
                               const uint8_t* d_img_l, const uint8_t* d_img_r, int channels, float* d_cost_l, float* d_cost_r,
                               int w, int h, int dminl, int dminr, int s_begin, int s_end, void* stream);
/* Host pointers, synchronous; mirrors smx_census_cost: the volume of i1 against i2 (u8 [h][w][channels]), size_d*w*h floats,
 * labels dmin + z.  With colour input the gray images for the codes come from smx_dev_rgb_to_grayscale with the default
 * smx_params. */
int smx_adcensus_cost(const smx_adcensus_params* p, const uint8_t* i1, const uint8_t* i2, int channels, float* cost, int w,
                      int h, int size_d, int dmin);
/* The AD-Census cost of this context.  Non-NULL switches it on and replaces whatever smx_ctx_set_cost chose; NULL switches it
 * off again (the reference's cost), and so does a later smx_ctx_set_cost.  (A setter of its own: smx_ctx_set_cost takes
 * SMX_COST_REFERENCE and SMX_COST_CENSUS only.)  The flows are those of the census cost: codes once per pair, then cost chunk ->
 * aggregation (the gray walkers, the colour-guided filter, SGM with the whole volumes); cost_l / cost_r of smx_pair_out
 * receive the AD-Census volumes.  With colour 0 it runs through smx_ctx_stereo_pair, and through smx_ctx_stereo_pair_rgb with
 * the AD term from the converted gray images.  With colour 1 it runs through smx_ctx_stereo_pair_rgb only, with either guide;
 * smx_ctx_stereo_pair returns SMX_E_ARG.  smx_ctx_stereo_pair_async returns SMX_E_ARG while it is on.  The table and the
 * buffers are allocated on first use. */
int smx_ctx_set_adcensus(smx_ctx* ctx, const smx_adcensus_params* p);

/* ------------------------------------------------------------------------------------
 * Mutual-information matching cost (Hirschmueller's HMI; not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The reference's cost and the AD term need equal gray values in the two views, census needs equal local ORDER.  Mutual
 * information (Hirschmueller, PAMI 2008) needs only that SOME fixed relation holds between the gray values of corresponding
 * pixels -- an inverted image, a folded tone curve, another modality -- and learns it from the pair itself: a joint histogram of
 * the pixels a disparity map pairs up gives a 256 x 256 table, and the cost of a cell is one lookup in it.
 * tests/mi_ref.py is this definition in numpy; histogram, table and volume equal it bit for bit.
 *   histogram  H, u32 [256][256], of a left map (f32 [h][w] holding integers that fit an int) with an occlusion mark:
 *         pixel (y, x) counts iff map[y][x] != mark and 0 <= xx < w with xx = x + (int)map[y][x]; it adds 1 to
 *         H[L[y][x]][R[y][xx]].  Integer sums: the same bits whatever the order of the atomics.
 *   table  T, u8 [256][256], from H on the host in double, every operation rounded on its own (no contraction), with
 *         g = {1, 6, 15, 20, 15, 6, 1} / 64 and conv(v)[j] = sum over t = 0 .. 6, ascending from 0.0, of g[t] * v[j + t - 3],
 *         v taken as 0.0 outside 0 .. 255; conv2(M) = conv along k of every row (the second index) first, then conv along i:
 *           n = sum of H (u64);  n == 0: T = 0 everywhere.        P[i][k] = (double)H[i][k] / (double)n
 *           h12 = conv2(-log(max(conv2(P), 1e-12)))
 *           p1[i] = sum over k ascending of P[i][k], p2[k] = sum over i ascending of P[i][k]
 *           h1 = conv(-log(max(conv(p1), 1e-12))), h2 the same from p2
 *           c[i][k] = (h12[i][k] - h1[i]) - h2[k];  c -= min c;  m = max c;  m == 0: T = 0 everywhere, else
 *           T[i][k] = (uint8_t)rint((c[i][k] * 255.0) / m)                   (ties to even)
 *         log is the C library's.  Hirschmueller's factor 1/n is absorbed by the normalisation to 0 .. 255: integers in the
 *         value set of the comb walker's exactness argument (no fall-back) and of SGM's clamp.
 *   cost  of view v, slice z: d = dmin_v + z, xx = x + d.  If 0 <= xx < w: the left view has
 *         cost[z][y][x] = (float)T[L[y][x]][R[y][xx]], the right view cost[z][y][x] = (float)T[L[y][xx]][R[y][x]]; else
 *         255.0f.  Layout, slice placement and [s_begin, s_end) as for smx_dev_census_cost_pair. */
#define SMX_MI_INIT_RANDOM 0
#define SMX_MI_INIT_REFERENCE 1
#define SMX_MI_LEVELS 256
typedef struct smx_mi_params {
    int iterations;   /* tables computed per pair, default 3; 1 .. 16 */
    int init;         /* SMX_MI_INIT_RANDOM (default) | SMX_MI_INIT_REFERENCE */
    uint32_t seed;    /* for the random start, default 0 */
} smx_mi_params;
void smx_default_mi_params(smx_mi_params* p);
/* The table of a histogram (both SMX_MI_LEVELS^2 entries).  Host only: works without a GPU. */
int smx_mi_table(const uint32_t* hist, uint8_t* table);
/* The same into device memory (d_table: SMX_MI_LEVELS^2 bytes, 16-byte aligned): a set-up call that copies from host memory
 * and waits for the copy on `stream`.  NOT graph-capturable. */
int smx_dev_mi_table(const uint32_t* hist, uint8_t* d_table, void* stream);
/* The histogram of d_map (with its occlusion mark) over the gray pair into d_hist, which the call zeroes first: a memset and
 * one launch on `stream`, no allocation, no synchronisation (graph-capturable).  w, h >= 1, w*h < 2^31. */
int smx_dev_mi_histogram(const uint8_t* d_img_l, const uint8_t* d_img_r, const float* d_map, float occlusion_mark,
                         uint32_t* d_hist, int w, int h, void* stream);
/* The random start map of a pair: d_map[y][x] = (float)(dmin + hash(seed, y*w + x) % size_d), the hash being the counter-based
 * one of PatchMatch stereo with view 0 and draw 0 (smx_pm_hash).  One launch, graph-capturable. */
int smx_dev_mi_random_map(float* d_map, int w, int h, int dmin, int size_d, uint32_t seed, void* stream);
/* Slices [s_begin, s_end) of the left volume (labels dminl + z) into d_cost_l and of the right volume (labels dminr + z) into
 * d_cost_r from d_table (as smx_dev_mi_table left it), both in one launch; either cost pointer may be NULL (not both).  One
 * launch, no allocation, no synchronisation (graph-capturable).  w, h >= 1. */
int smx_dev_mi_cost_pair(const uint8_t* d_table, const uint8_t* d_img_l, const uint8_t* d_img_r, float* d_cost_l,
                         float* d_cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end, void* stream);
/* Host pointers, synchronous.  smx_mi_histogram: the histogram of a left map.  smx_mi_cost mirrors smx_census_cost: the
 * volume of view `right` (0: i1 is the left image and i2 the right one; 1: i1 is the right image, i2 the left one, and the
 * table is read with the roles swapped), size_d*w*h floats, labels dmin + z. */
int smx_mi_histogram(const uint8_t* img_l, const uint8_t* img_r, const float* map, float occlusion_mark, uint32_t* hist,
                     int w, int h);
int smx_mi_cost(const uint8_t* table, const uint8_t* i1, const uint8_t* i2, int right, float* cost, int w, int h, int size_d,
                int dmin);

#define SMX_COST_MI 2   /* what smx_ctx_set_mi selects; smx_ctx_set_cost does not take it */
/* The mutual-information cost of this context.  Non-NULL switches it on and replaces whatever smx_ctx_set_cost or
 * smx_ctx_set_adcensus chose; NULL switches it off again (the reference's cost), and so does a later smx_ctx_set_cost or
 * smx_ctx_set_adcensus.  Valid: 1 <= iterations <= 16, init one of the two above.  A pair with it on runs, in order:
 *   1. the start map: SMX_MI_INIT_RANDOM is smx_dev_mi_random_map(dminl, size_d, seed), every pixel valid;
 *      SMX_MI_INIT_REFERENCE is the LR-checked left map (`occlusion`) of one pass of the pair with the reference's cost;
 *   2. for k = 1 .. iterations: the histogram of the current map (occlusion mark dminl - 100), its table on the host (one
 *      round trip), then the pair in the flows of the census cost (cost chunk -> aggregation) with the MI cost of that table.
 *      The current map of the next iteration is this pass's LR-checked left map (`occlusion`).
 * The start pass and the passes before the last stop behind the LR check and the fill: uniqueness, speckle removal, region
 * voting, sub-pixel and the adjustment run in the last pass only, so their invalidations never reach a histogram.  Every
 * output, cost_l / cost_r included, is the last pass's.  With cross-scale aggregation the levels take the table of level 0.
 * It runs in every flow the census cost runs in (not with PatchMatch stereo); smx_ctx_stereo_pair_async returns SMX_E_ARG
 * while it is on.  The table and the buffers are allocated on first use. */
int smx_ctx_set_mi(smx_ctx* ctx, const smx_mi_params* p);
/* The table of the last pass of the last synchronous pair and the histogram it came from (either may be NULL); SMX_E_ARG if
 * that pair ran without the mutual-information cost. */
int smx_ctx_mi_table(smx_ctx* ctx, uint8_t* table, uint32_t* hist);

/* ------------------------------------------------------------------------------------
 * ZNCC window matching cost: zero-mean normalised cross-correlation (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The reference's cost and the AD term need equal gray values, census keeps no magnitudes, mutual information learns ONE global
 * relation between the gray values of the two views.  Zero-mean normalised cross-correlation over a window (among the core
 * costs of Hirschmueller & Scharstein, PAMI 2009) is invariant to a LOCAL affine change a*I + b, a > 0 -- vignetting, an
 * exposure gradient, a light that moved between the exposures -- and keeps the magnitudes inside the window.
 * tests/zncc_ref.py is this definition in numpy; moments and volumes equal it bit for bit.
 *   window  (2 rx + 1) x (2 ry + 1), N pixels, 1 <= rx, ry <= 4 (N <= 81); images replicate-clamped as for census:
 *         A_ext[y][x] = A[clamp(y, 0, h-1)][clamp(x, 0, w-1)].  An image smaller than the window is legal.
 *   moments of an image I at (y, x), exact integers: S = sum of I_ext over the window, Q = sum of I_ext^2,
 *         V = N Q - S^2, 0 <= V <= 81 * 81 * 65025 < 2^31.  One 8-byte word a pixel: S | (uint64_t)V << 32.
 *   cost  of view v, slice z, A the view's own image and B the other's: d = dmin_v + z, xx = x + d.
 *         xx < 0 or xx >= w:                  cost = 255.0f
 *         else P = sum over the window of A_ext[y+dy][x+dx] * B_ext[y+dy][xx+dx]      (each image clamped on its own)
 *              num = N P - S_A(y, x) S_B(y, xx)   (|num| < 2^31),   Va = V_A(y, x), Vb = V_B(y, xx)
 *         Va == 0 or Vb == 0 (a flat window): cost = 128.0f
 *         else, in f32, every operation rounded on its own (no contraction), int -> float to nearest-even:
 *              nf = (float)|num|;  s = min((nf * nf) / ((float)Va * (float)Vb), 1.0f)
 *              cost = rintf(num >= 0 ? 127.5f * (1.0f - s) : 127.5f * (1.0f + s))                       (ties to even)
 *         That is 127.5 (1 - rho |rho|) with rho the ZNCC: the signed square is monotone in rho and needs no square root, only
 *         the correctly rounded f32 multiply and divide.  Costs are integers 0 .. 255: the value set of the comb walker's
 *         exactness argument (no fall-back) and of SGM's clamp.
 *   Layout [z][y][x], slice placement and [s_begin, s_end) as for smx_dev_census_cost_pair. */
typedef struct smx_zncc_params {
    int rx, ry;       /* window radii, default 3, 3; 1 .. 4 each */
} smx_zncc_params;
void smx_default_zncc_params(smx_zncc_params* p);
/* N of the window, or SMX_E_ARG (negative) for invalid parameters.  Host only: works without a GPU. */
int smx_zncc_window(const smx_zncc_params* p);
/* Columns and rows of a workgroup's tile of smx_dev_zncc_cost_pair (for tests that put sizes at a tile seam). */
int smx_zncc_geometry(int* cols, int* rows);
/* The moments of `nimages` planes of w x h that lie back to back at d_img into d_mom (nimages * w * h words, 8-byte aligned):
 * one launch, no allocation, no synchronisation (graph-capturable).  w, h >= 1. */
int smx_dev_zncc_moments(const smx_zncc_params* p, const uint8_t* d_img, uint64_t* d_mom, int w, int h, int nimages,
                         void* stream);
/* Slices [s_begin, s_end) of the left volume (labels dminl + z) into d_cost_l and of the right volume (labels dminr + z) into
 * d_cost_r from d_mom ([2][h][w]: the left image's moments, then the right one's, of the same parameters) and the two images,
 * both in one launch; either cost pointer may be NULL (not both).  No allocation, no synchronisation (graph-capturable). */
int smx_dev_zncc_cost_pair(const smx_zncc_params* p, const uint64_t* d_mom, const uint8_t* d_img_l, const uint8_t* d_img_r,
                           float* d_cost_l, float* d_cost_r, int w, int h, int dminl, int dminr, int s_begin, int s_end,
                           void* stream);
/* Host pointers, synchronous; mirrors smx_census_cost: the volume of i1 against i2, size_d*w*h floats, labels dmin + z. */
int smx_zncc_cost(const smx_zncc_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h, int size_d,
                  int dmin);

#define SMX_COST_ZNCC 3   /* what smx_ctx_set_zncc selects; smx_ctx_set_cost does not take it */
/* The ZNCC cost of this context.  Non-NULL switches it on and replaces whatever smx_ctx_set_cost, smx_ctx_set_adcensus or
 * smx_ctx_set_mi chose; NULL switches it off again (the reference's cost), and so does a later call of one of those setters.
 * A pair with it on runs the moments of both images once, then cost chunk -> aggregation in every flow the census cost runs in
 * (not with PatchMatch stereo); cost_l / cost_r of smx_pair_out receive the ZNCC volumes.  smx_ctx_stereo_pair_async returns
 * SMX_E_ARG while it is on.  The moments live in the buffer of the census codes, allocated on first use. */
int smx_ctx_set_zncc(smx_ctx* ctx, const smx_zncc_params* p);

/* ------------------------------------------------------------------------------------
 * Cross-based aggregation: colour-adaptive support regions (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* Cross-based aggregation (Zhang, Lu, Lafruit 2009), the step of Mei et al. 2011 between the AD-Census cost and the scan-line
 * optimiser: every pixel gets a support region that grows up to l1 pixels in each direction through similar colour and stops
 * dead at a colour edge; it is built once per view from the guide alone and applied to every slice with two passes of sums.
 * Everything is an exact integer, so the result is the same bits in every run and under every schedule.
 * tests/cross_ref.py is this definition in numpy; the result equals it bit for bit.
 * Defaults (Mei's values): l1 34, l2 17, tau1 20, tau2 6, iterations 4.  Valid: 1 <= l1 <= 63, 0 <= l2 <= l1,
 * 1 <= tau2 <= tau1 <= 256, 1 <= iterations <= 4; anything else is SMX_E_ARG before any device call.
 *   guide:   u8 [h][w][channels], channels 1 (gray), 3 or 4 (a fourth byte is ignored); D(p, q) = max over the channels c of
 *            |I_c(p) - I_c(q)|.
 *   arms:    for a pixel p and a direction e (left, right, up, down) the largest k in 0 .. l1 such that every j = 1 .. k has,
 *            with q_j = p + j e: q_j inside the image, D(q_j, p) < tau1, D(q_j, q_{j-1}) < tau1, and D(q_j, p) < tau2 where
 *            j > l2.  The comparisons are strict (tau = 256 accepts everything); an arm may be 0.  One u32 per pixel holds the
 *            four arms: l | r << 8 | u << 16 | d << 24.
 *   values:  a cost c is read through the clamp of smx_dev_sgm_wta_pair, C = c >= 0 ? (c <= 255 ? (int)c : 255) : 0 (a NaN
 *            gives 0: the call is total on any bits); V_0 = 16 * C, four fractional bits.
 *   iteration i = 0 .. iterations - 1: even i sums horizontally first,
 *              H(y, x) = sum of V(y, x') over x - l(y, x) <= x' <= x + r(y, x),
 *              S(y, x) = sum of H(y', x) over y - u(y, x) <= y' <= y + d(y, x);
 *            odd i vertically first: T(y, x) = the sum of V over the vertical arm of (y, x), S(y, x) = the sum of T(y, x') over
 *            the horizontal arm of (y, x).  area_HV / area_VH are the same sums of V = 1 (1 .. 127^2).  With `area` the area of
 *            the iteration's order, in floor division: V_{i+1} = (2 S + area) / (2 area).  V <= 4080 and S < 2^26 always.
 *   output:  q = (float)V_iterations * 0.0625f (exact).
 *   winner:  the packed keys and the tie rule of smx_dev_aggregate_wta (the last slice of equal costs wins).
 *
 * smx_dev_cross_arms: the arms planes of the guides, n u32 each, the left view's first; either guide may be NULL (not both),
 * which leaves the one plane.  One launch.
 * smx_dev_cross_wta_pair has the shape and the rules of smx_dev_cgf_wta_pair: both views in every launch; either guide / cost
 * pair may be NULL (not both; a view's guide and cost come together) for the one-view form, whose outputs hold that one view;
 * the cost slices [s_begin, s_end) materialised at d_cost[(s - s_begin) * w*h]; d_keys IN/OUT, accumulated across calls and
 * D-shards by the int64 min; d_agg optional, (s_end - s_begin) * n floats per view: q; d_nbr, d_uq optional, 3n floats per
 * view each, with their rule (ascending, contiguous ranges on one set of keys).  The slices go in chunks that fit the workspace
 * (smx_set_max_slices_per_launch bounds the chunk as well); the chunking does not change a bit.  Five launches per call for
 * the support regions, then per chunk two per iteration and the winner-take-all pass; no allocation, no synchronisation
 * (graph-capturable).  smx_cross_workspace_bytes(w, h, nslices, nviews) holds `nslices` slices in flight: per view and pixel
 * 8 bytes of arms and areas and, per slice in flight, 12 bytes (two u16 planes, the u32 sums between an iteration's two
 * passes, one f32 plane), plus 255 bytes (0 for invalid sizes: w, h >= 1, w*h < 2^31, nslices >= 1, nviews 1 or 2).  Fewer
 * bytes than for one slice is SMX_E_WS before anything is launched.  The memory contract is that of the aggregation entries
 * above smx_agg_workspace_bytes: nothing is written outside the workspace and the stated extents, the workspace may hold
 * anything and needs no alignment, the inputs are not modified.
 * smx_cross_aggregate: host pointers, one view, synchronous; filter_cost / disp_map IN/OUT and agg as for
 * smx_colour_guided_filter. */
typedef struct smx_cross_params { int l1, l2, tau1, tau2, iterations; } smx_cross_params;
void smx_default_cross_params(smx_cross_params* p);
size_t smx_cross_workspace_bytes(int w, int h, int nslices, int nviews);
int smx_dev_cross_arms(const smx_cross_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels, int w, int h,
                       uint32_t* d_arms, void* stream);
int smx_dev_cross_wta_pair(const smx_cross_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels,
                           const float* d_cost_l, const float* d_cost_r, int w, int h, int s_begin, int s_end, int64_t* d_keys,
                           float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_cross_aggregate(const smx_cross_params* p, const uint8_t* guide, int channels, const float* cost, float* filter_cost,
                        float* disp_map, float* agg, int w, int h, int size_d, int dmin);
/* Cross-based aggregation of this context.  Non-NULL switches it on, NULL switches it off again (the guided filter).  (A
 * setter of its own: smx_ctx_set_aggregation takes SMX_AGG_GUIDED and SMX_AGG_SGM only.)  The flow is that of the colour
 * guide: cost chunk -> smx_dev_cross_wta_pair, the cost being the reference's, census or AD-Census.  The guide is the gray
 * pair through smx_ctx_stereo_pair and the colour images through smx_ctx_stereo_pair_rgb.  mean_l / mean_r are not produced
 * (SMX_E_ARG if requested).  Together with SMX_AGG_SGM or SMX_GUIDE_RGB the pair call returns SMX_E_ARG, and so does
 * smx_ctx_stereo_pair_async while it is on.  The workspace and the chunk buffers are allocated on first use. */
int smx_ctx_set_cross(smx_ctx* ctx, const smx_cross_params* p);

/* ------------------------------------------------------------------------------------
 * Region voting and 16-direction interpolation on the cross arms (not a stage of the reference; opt-in, behind speckle removal)
 * ---------------------------------------------------------------------------------- */

/* The outlier refinement of Mei et al. 2011 on the support regions of smx_dev_cross_arms: an invalid pixel takes the most
 * frequent valid label of its own cross region (iterative region voting), what is left looks along 16 directions for its
 * nearest valid pixels (proper interpolation), and what neither reaches is left to the scan-line fill.  Integers only: the
 * result is the same bits in every run and under every schedule.  tests/vote_ref.py is this definition in numpy; the result
 * equals it bit for bit.
 *
 * Inputs.
 *   disp     f32 [h][w]: the left map behind the LR check, uniqueness and speckle stages
 *   arms     u32 [h][w], as smx_dev_cross_arms packs them (l | r << 8 | u << 16 | d << 24).  A region is cut at the image
 *            border whatever its arms say (the arms of smx_dev_cross_arms never reach across it).
 *   guide    u8 [h][w][channels], channels 1, 3 or 4, a fourth byte ignored, with the cross aggregation's D(p, q); read for
 *            the mismatches only: it may be NULL with interpolate == 0 or disp_r == NULL
 *   disp_r   optional f32 [h][w]: the right WTA map
 *   dmin, size_d   the label range
 *   d_lr     from smx_params
 *
 * Which pixels are valid and which vote.
 *   valid:   a pixel is valid iff it "counts" by the speckle filter's rule with vmin = (float)dmin: finite and
 *            (float)(int)disp[p] >= vmin, with the truncation and saturation written there.
 *   outlier: every other pixel.
 *   voter:   a valid pixel votes iff its bin b = (int)disp[p] - dmin lies in 0 .. size_d - 1.  A valid pixel outside that
 *            range stays as it is and casts no vote.
 *   The call is total on any bits: NaN, +-inf, -0, fractions, values beyond int.
 *
 * Region of p = (y, x): the aggregation's horizontal-first region, all (y', x') with y - u(p) <= y' <= y + d(p) and
 * x - l(y', x) <= x' <= x + r(y', x).  With every pixel a voter its count is area_HV.
 *
 * Voting, `iterations` rounds.  The rounds are Jacobi: round k reads map M_k only and writes M_{k+1}, with M_0 = disp.
 *   For an outlier p of M_k, H_p(b) is the number of voters of M_k in its region with bin b, and S_p the sum over b.
 *   b* is the largest b among those with the largest count (the project's "last slice of equal costs wins").
 *   The vote is accepted iff S_p > tau_s and 100 * H_p(b*) > tau_h_pct * S_p, in exact integers.
 *   On acceptance M_{k+1}[p] = (float)(dmin + b*).  Every other pixel, a valid one included, is copied bit for bit.
 *
 * Interpolation: one pass over M_iterations as a snapshot; skipped with interpolate == 0.
 *   directions: for every remaining outlier p and each of the 16 directions, in this order: (dx, dy) = (1,0), (2,1), (1,1),
 *               (1,2), (0,1), (-1,2), (-1,1), (-2,1), (-1,0), (-2,-1), (-1,-1), (-1,-2), (0,-1), (1,-2), (1,-1), (2,-1).
 *   candidate:  the candidate of a direction is the first q_j = p + j (dx, dy), j = 1, 2, ..., inside the image that is a voter.
 *   mismatch:   p is a mismatch iff disp_r is given and some s in 0 .. size_d - 1 has, with d = dmin + s, 0 <= x + d < w and
 *               fabsf((float)d + disp_r[y][x + d]) <= d_lr: the LR check's own test and sign convention, in f32.  A NaN fails it.
 *   occlusion:  every other remaining outlier.  With disp_r == NULL every outlier is one.
 *   value:      an occlusion takes the largest candidate value, which is the background as fill_occlusion sees it (of equal
 *               values, +0 and -0 among them, the first in the order above).  A mismatch takes the candidate with the smallest
 *               D(p, q), the first in the order above among equals.  The candidate's bits are copied.
 *   no candidate: the pixel is copied unchanged.
 *
 * Defaults (tau_s, tau_h_pct, iterations: Mei's values): tau_s 20, tau_h_pct 40, iterations 5, interpolate 1.  Valid:
 * tau_s >= 0, 0 <= tau_h_pct <= 99, 0 <= iterations <= 8, interpolate 0 or 1, 1 <= size_d <= 512, channels 1, 3 or 4,
 * w, h >= 1, w*h < 2^31; anything else is SMX_E_ARG before any device call.
 *
 * smx_dev_region_vote: device pointers; max(iterations, 1) + 1 kernel launches on `stream` (one per round -- a copy where there
 * is none -- and the interpolation, which with interpolate == 0 is the copy into d_out), no allocation, no synchronisation
 * (graph-capturable).  d_out == d_disp is allowed.  The memory contract is that of the other stages: nothing is written outside
 * [0, smx_vote_workspace_bytes(w, h)) of d_ws (two maps of n floats plus 255 bytes; 0 for invalid w, h) and the w*h floats of
 * d_out; the workspace may hold anything and needs no alignment; a smaller one is SMX_E_WS before any launch; the inputs are
 * not modified.
 * smx_region_vote: host pointers, synchronous; it builds the arms from cross' l1, l2, tau1, tau2 (iterations ignored; NULL:
 * the defaults) with smx_dev_cross_arms on `guide`, which it therefore needs always. */
typedef struct smx_vote_params { int tau_s, tau_h_pct, iterations, interpolate; } smx_vote_params;
void smx_default_vote_params(smx_vote_params* p);
size_t smx_vote_workspace_bytes(int w, int h);
int smx_dev_region_vote(const smx_vote_params* p, const uint32_t* d_arms, const uint8_t* d_guide, int channels, const float* d_disp,
                        const float* d_disp_r, float* d_out, int w, int h, int dmin, int size_d, int d_lr, void* d_ws,
                        size_t ws_bytes, void* stream);
int smx_region_vote(const smx_vote_params* p, const smx_cross_params* cross, const uint8_t* guide, int channels, const float* disp,
                    const float* disp_r, float* out, int w, int h, int dmin, int size_d, int d_lr);
/* Test hook, NOT part of the stable contract (it may change or go with the kernels): the tile of the voting kernel (columns,
 * rows), so that the tests put their shapes and outliers on the seams between tiles. */
int smx_vote_geometry(int* tile_cols, int* tile_rows);
/* Region voting of this context.  vote NULL switches it off (the default); cross NULL means smx_default_cross_params (its
 * iterations are ignored).  While it is on, smx_ctx_stereo_pair / _rgb builds the arms of the left guide -- the gray left image,
 * or the colour one through the _rgb entry -- and runs smx_dev_region_vote behind LR check -> uniqueness -> speckle removal,
 * with the right winner-take-all map as disp_r; out->filled becomes the scan-line fill of the voted map.  The validity map is
 * NOT replaced: the sub-pixel fit's test and wmf "occluded" keep taking the map they take without it, so a voted pixel gets no
 * sub-pixel offset (its label is not its winner's) and stays a pixel for the weighted median to refine.  It works with every
 * aggregation and every cost.  smx_ctx_stereo_pair_async returns SMX_E_ARG while it is on.  smx_ctx_vote_map copies the voted
 * map of the last synchronous pair of the context (n floats); SMX_E_ARG if that pair ran without it.  Buffers are allocated on
 * first use. */
int smx_ctx_set_vote(smx_ctx* ctx, const smx_vote_params* vote, const smx_cross_params* cross);
int smx_ctx_vote_map(smx_ctx* ctx, float* voted);

/* ------------------------------------------------------------------------------------
 * Scan-line optimisation with colour-adaptive penalties (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The scan-line optimiser of Mei et al. 2011, the step between the cross-based aggregation and the winners: the recurrence of
 * smx_dev_sgm_wta_pair with penalties that are lowered where the step of a path crosses a colour edge in BOTH views, which is
 * where a real depth step is.  A constant p2 large enough to carry a weakly textured surface through its noise erases a thin
 * foreground object (entering and leaving it costs 2 p2); lowered at the object's colour edges it does not.
 * tests/scanline_ref.py is this definition in numpy; the result equals it bit for bit.
 * Defaults: p1 127, p2 382, tau_so 15, paths 4 (Mei's Pi1 = 1.0, Pi2 = 3.0, tau_SO = 15 and four directions, at the AD-Census
 * default scale of 127.5).  Valid: 0 <= p1 <= p2 <= 4095, 1 <= tau_so <= 256, paths 4 or 8; w, h >= 1, w*h < 2^31,
 * 1 <= size_d <= SMX_SGM_MAX_D, channels 1, 3 or 4, any int for dminl / dminr; anything else is SMX_E_ARG before any device call.
 *   costs, directions, restart rule, tie rule, d_keys (OUT only), d_agg, d_nbr, d_uq: those of smx_dev_sgm_wta_pair (_uq); the
 *            directions in the order (1,0) (-1,0) (0,1) (0,-1) (1,1) (-1,1) (1,-1) (-1,-1), the first four for paths 4.  A cost is
 *            read through the clamp C = c >= 0 ? (c <= 255 ? (int)c : 255) : 0, so the q of smx_dev_cross_wta_pair, which has four
 *            fractional bits, is truncated to its integer part.  d_uq is optional here (NULL, or 3n floats per view).
 *   guides:  u8 [h][w][channels]; D(p, q) = the maximum over the first three channels of |I_c(p) - I_c(q)|, the distance of
 *            smx_dev_cross_arms (a fourth byte is ignored).
 *   flags:   for a view v, a pixel p = (x, y), a direction r and a slice z the label is d = dmin_v + z and the partner of p is
 *            q = (x + d, y) in the OTHER view (the convention of the cost entries).
 *              e1 = [D_own(p, p - r) >= tau_so]
 *              e2 = [D_other(q, q - r) >= tau_so] if q and q - r both lie inside the image, else 0
 *              k  = e1 + e2: e2 depends on z, so the penalties are per label.  tau_so = 256 never flags an edge.
 *   penalties of (p, z): (P1, P2) = (p1, p2) for k = 0, (p1 / 4, p2 / 4) for k = 1, (p1 / 10, p2 / 10) for k = 2, in floor division.
 *   recurrence: L_r(p, z) = C(p, z) where p - r lies outside the image; otherwise, with m = min_j L_r(p - r, j),
 *              L_r(p, z) = C(p, z) + min(L_r(p-r, z), L_r(p-r, z-1) + P1, L_r(p-r, z+1) + P1, m + P2) - m
 *            with the terms of z - 1 < 0 and z + 1 >= size_d left out.  P2 <= 4095, so the bounds of smx_dev_sgm_wta_pair hold: S
 *            fits u16, (float)S is exact, and the result is the same bits in every run.  With tau_so = 256 the outputs equal
 *            smx_dev_sgm_wta_pair's bit for bit.
 * smx_dev_scanline_wta_pair: BOTH guides are always required (a view's e2 reads the other guide); either cost pointer may be
 * NULL (not both), the one-view form, whose outputs hold that one view as for SGM.  A fixed sequence of kernel launches on
 * `stream` (the SGM sequence plus one: 6 for paths 4, 10 for paths 8), no allocation, no synchronisation (graph-capturable).
 * d_ws needs no alignment and may hold anything; fewer than smx_scanline_workspace_bytes(w, h, size_d, nviews) bytes is SMX_E_WS
 * before anything is launched (the SGM workspace plus, for each of the two views whatever nviews is, one byte per pixel of edge
 * flags with 8 bytes of padding a row; 0 for invalid sizes or nviews other than 1, 2).  Nothing is written outside the workspace
 * and the stated extents; the inputs are not modified.
 * smx_scanline_optimize: host pointers, synchronous, one view with label offset dmin; guide_own is that view's guide, guide_other
 * the other view's.  agg, best, disp_map as for smx_sgm_aggregate. */
typedef struct smx_scanline_params { int p1, p2, tau_so, paths; } smx_scanline_params;
void smx_default_scanline_params(smx_scanline_params* p);
size_t smx_scanline_workspace_bytes(int w, int h, int size_d, int nviews);
int smx_dev_scanline_wta_pair(const smx_scanline_params* p, const uint8_t* d_guide_l, const uint8_t* d_guide_r, int channels,
                              const float* d_cost_l, const float* d_cost_r, int w, int h, int size_d, int dminl, int dminr,
                              int64_t* d_keys, float* d_agg, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_scanline_optimize(const smx_scanline_params* p, const uint8_t* guide_own, const uint8_t* guide_other, int channels,
                          const float* cost, float* agg, float* best, float* disp_map, int w, int h, int size_d, int dmin);
/* The scan-line optimiser of this context.  Non-NULL switches it on, NULL switches it off again.
 * Alone: the flow of SMX_AGG_SGM -- both whole cost volumes (the reference's, census or AD-Census), smx_dev_scanline_wta_pair,
 * then the usual finish; agg_l / agg_r receive S.
 * With smx_ctx_set_cross on: the chain of Mei et al.  smx_dev_cross_wta_pair runs over its chunks with its q collected into two
 * whole volumes and its keys discarded, then the optimiser runs on those volumes.  It reads them through the clamp, so the four
 * fractional bits of q are truncated; agg_l / agg_r receive S, not q.
 * The guide is the gray pair through smx_ctx_stereo_pair and the colour pair through smx_ctx_stereo_pair_rgb.  The uniqueness,
 * speckle, vote, sub-pixel stages run behind it unchanged.  mean_l / mean_r are not produced (SMX_E_ARG if requested).  Together
 * with SMX_AGG_SGM or SMX_GUIDE_RGB, or with more than SMX_SGM_MAX_D labels, the pair call returns SMX_E_ARG, and so does
 * smx_ctx_stereo_pair_async while it is on.  The workspace and the volumes are allocated on first use. */
int smx_ctx_set_scanline(smx_ctx* ctx, const smx_scanline_params* p);

/* ------------------------------------------------------------------------------------
 * Depth-discontinuity adjustment of a label map from the aggregated costs (not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The depth-discontinuity adjustment of Mei et al. 2011, the step between the interpolation and the sub-pixel fit: a pixel
 * beside a step of the label map takes a neighbour's label where the aggregated volume says that label costs it less.  The
 * stages behind the winner-take-all pass put labels in without asking the costs (the vote, the interpolation, the fill); at a
 * depth step the fill carries one surface's label across the band that the LR check rejected, and this stage moves the edge
 * back to where the costs have it.  Integers and comparisons only, apart from the one f32 formula of the sub-pixel map: the
 * result is the same bits in every run.  tests/adjust_ref.py is this definition in numpy; the result equals it bit for bit.
 *
 * Inputs.
 *   disp     f32 [h][w]: a label map of one view (n = w*h floats)
 *   A        f32 [size_d][h][w]: that view's aggregated volume, the layout of d_agg / agg_l of every aggregation
 *   dmin, size_d   the label range
 *
 * Labelled pixel: p is labelled iff disp[p] is finite, integer-valued and 0 <= disp[p] - dmin < size_d; its slice is
 *   z(p) = disp[p] - dmin.  The LR marker dmin - 100, NaN, +-inf and fractional values are not labelled; -0 is the label 0.  An
 *   unlabelled pixel is copied bit for bit and is nobody's candidate.
 * Candidates of a labelled p = (x, y), in this order: (x-1, y), (x+1, y) and, with vertical == 1, (x, y-1), (x, y+1); only those
 *   that lie inside the image, are labelled and have |z(q) - z(p)| >= tau_e, in integers.  A pixel without a candidate is
 *   copied bit for bit: it is not on a discontinuity.
 * Choice: best = A[z(p)][p]; for each candidate q in order, if A[z(q)][p] < best (plain f32 comparison, false for a NaN) then
 *   best = A[z(q)][p] and p takes disp[q], the candidate's bits.  The own label wins ties, among equal candidates the first
 *   wins, a NaN cost never wins and a NaN own cost is never replaced.
 * Rounds: `iterations` Jacobi rounds, each reads the map of the round before as a snapshot and writes another.  A pixel changed
 *   in round k is a candidate in round k + 1, so an edge moves at most one pixel a round.  A pixel's own cost never rises.
 *   There is no early exit.
 * Sub-pixel map: d_sub NULL, or n floats IN/OUT with subpix_mode SMX_SUBPIX_PARABOLA or SMX_SUBPIX_EQUIANGULAR.  A pixel whose
 *   final label differs from its input label gets sub[p] = out[p] + smx_subpixel_delta(mode, A[z'][p], A[z'-1][p], A[z'+1][p])
 *   with z' its final slice and NaN for a neighbour outside 0 .. size_d - 1 (delta 0 then); every other pixel of d_sub is left
 *   untouched.  With d_sub NULL subpix_mode must be 0 or one of the two.
 *
 * Defaults: tau_e 2, vertical 1, iterations 1 (Mei's single pass).  Valid: 1 <= tau_e <= 512, vertical 0 or 1,
 * 1 <= iterations <= 8, 1 <= size_d <= 512, w, h >= 1, w*h < 2^31, any int for dmin; anything else is SMX_E_ARG before any
 * device call.
 *
 * smx_dev_discontinuity_adjust: device pointers; `iterations` kernel launches on `stream`, and in front of them one
 * device-to-device copy of the map into the workspace where d_out == d_disp (the only overlap allowed); no allocation, no
 * synchronisation (graph-capturable).  Nothing is written outside [0, smx_adjust_workspace_bytes(w, h)) of d_ws (two maps of n
 * floats plus 255 bytes; 0 for invalid w, h), the n floats of d_out and the changed pixels of d_sub; the workspace may hold
 * anything and needs no alignment; a smaller one is SMX_E_WS before any launch; d_agg is not modified, and d_disp only as d_out.
 * smx_discontinuity_adjust: host pointers, synchronous; sub NULL or n floats IN/OUT. */
typedef struct smx_adjust_params { int tau_e, vertical, iterations; } smx_adjust_params;
void smx_default_adjust_params(smx_adjust_params* p);
size_t smx_adjust_workspace_bytes(int w, int h);
int smx_dev_discontinuity_adjust(const smx_adjust_params* p, const float* d_disp, const float* d_agg, float* d_out, int w, int h,
                                 int dmin, int size_d, int subpix_mode, float* d_sub, void* d_ws, size_t ws_bytes, void* stream);
int smx_discontinuity_adjust(const smx_adjust_params* p, const float* disp, const float* agg, float* out, int w, int h, int dmin,
                             int size_d, int subpix_mode, float* sub);
/* Test hook, NOT part of the stable contract (it may change or go with the kernel): the footprint of a workgroup of the round
 * kernel (columns, rows), so that the tests put their shapes and depth steps on the seams between workgroups. */
int smx_adjust_geometry(int* cols, int* rows);
/* The adjustment of this context.  NULL switches it off (the default).  While it is on, smx_ctx_stereo_pair / _rgb keeps the
 * aggregated volumes as when agg_l is requested, through whichever aggregation is set (every aggregation of the context
 * delivers whole volumes: the guided filter, SGM, the colour guide, cross-based aggregation, the scan-line optimiser and the
 * chain), and runs smx_dev_discontinuity_adjust on the filled left map with the left volume, behind LR check -> uniqueness ->
 * speckle -> vote -> fill -> sub-pixel fit: out->filled becomes the adjusted map, and with smx_ctx_set_subpixel on the
 * context's sub-pixel filled map carries the changed pixels' own fits.  The validity map is NOT replaced.  A context of more than
 * 512 labels cannot deliver the stage its label range: the setter returns SMX_E_ARG with a message (the pair call checks it
 * again).  smx_ctx_stereo_pair_async returns SMX_E_ARG while it is on.  Buffers are allocated on first use. */
int smx_ctx_set_adjust(smx_ctx* ctx, const smx_adjust_params* p);

/* ------------------------------------------------------------------------------------
 * Cross-scale cost aggregation (Zhang et al., CVPR 2014; not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* A window filter fails on textureless surfaces wider than its window.  Cross-scale aggregation is the guided filter's own
 * remedy: the pair is aggregated at every level of an image pyramid with the UNCHANGED aggregation, and a quadratic inter-scale
 * regulariser ties the levels together.  Its closed form makes the regularised finest cost a fixed linear combination of the
 * levels' aggregated costs at the pixel's and the label's ancestors.  tests/cscale_ref.py is this definition in numpy; the
 * results equal it bit for bit.
 *
 * Parameters.  scales: 1 .. SMX_CSCALE_MAX_SCALES levels (1 = level 0 alone); lambda: the regulariser's weight, finite and >= 0.
 * Defaults 4 and 1.0; the paper runs 5 scales and lambda = 0.3 with small windows.  Anything else is SMX_E_ARG before any device
 * call.
 *
 * Pyramid.  pyr_down of a u8 image [h][w][channels] (channels 1, 3 or 4, interleaved, each channel by itself) is
 * [(h+1)/2][(w+1)/2][channels]: taps 1 4 6 4 1 along x on integers without rounding, the same taps along y on those sums, taken
 * at the even source coordinates, value (t + 128) >> 8.  Borders are reflect-101 (i < 0 -> -i, i >= N -> 2(N-1) - i), then
 * clamped to [0, N-1], which matters for N of 1 or 2.  Level s is pyr_down applied s times.  A level's gray image is the pyramid
 * of the level-0 gray image, not the gray of the level's colour image; the colour pyramid serves the colour guide and the
 * colour AD term only.
 *
 * Labels.  A view with labels dmin .. dmin + size_d - 1 has at level s the labels dmin_s .. dmax_s with dmin_s = dmin >> s and
 * dmax_s = (dmin + size_d - 1) >> s (arithmetic shifts: floor for negative labels), size_d_s = dmax_s - dmin_s + 1.
 * smx_cscale_level gives a level's geometry (s >= 0; SMX_E_ARG for w, h, size_d < 1 or s < 0 or s > 30).
 *
 * Per-level volumes.  A_s [size_d_s][h_s][w_s] is the aggregated volume of the level-s pair with labels dmin_s .. of the view,
 * from the same cost, aggregation and parameters at every level (the same radius, eps and thresholds, as in the paper).
 *
 * Weights.  M is the scales x scales tridiagonal matrix with -lambda beside the diagonal and 1 + lambda * (number of
 * neighbouring levels) on it; wt[s] = (float)(M^-1)[0][s], computed on the host in double by the Thomas elimination
 * (smx_cscale_weights writes `scales` floats).  lambda == 0 gives 1, 0, ...; they sum to 1.
 *
 * Combination.  For slice z and pixel (x, y) of level 0: t_s = wt[s] * A_s[((dmin + z) >> s) - dmin_s][y >> s][x >> s], each
 * product rounded to f32; out = t_0, then out = out + t_s for s = 1 .. scales-1 in this order, each sum rounded to f32, no fused
 * multiply-add.  A NaN or an infinity propagates as IEEE 754 says.  With scales == 1 (wt = 1) out equals A_0 bit for bit.
 *
 * Winners.  From out through the packed key's rule with the slices ascending: smallest cost, the last slice among equal costs,
 * a NaN never.
 *
 * What it cannot do: a label of level s stands for 2^s labels of level 0, so the coarse levels say nothing about which of those
 * is right.  Inside a textureless band the winners come to within 2^(scales-1) of the truth, not onto it; the sub-pixel fit and
 * the weighted median are the stages for the rest.
 *
 * smx_dev_pyr_down: one launch on `stream`; writes the ((w+1)/2) * ((h+1)/2) * channels bytes of d_dst and nothing else; d_src
 * and d_dst must not overlap.  w, h >= 1, w*h < 2^31.  smx_pyr_down: host pointers, synchronous.
 *
 * smx_dev_cscale_wta_pair: the combination and the winner-take-all pass over it in ONE launch on `stream`; no allocation, no
 * synchronisation (graph-capturable).  d_agg_l / d_agg_r: HOST arrays of `scales` device pointers, entry s the whole volume A_s
 * of that view (they are read during the call only); either may be NULL for a one-view call.  Outputs as in the other pair
 * entries: with both views the left view's first, the right view's behind it; the one view of a one-view call at the front.
 *   d_keys  OUT  int64 [views][h][w]: the packed keys of out (written fresh: what the buffer held is ignored)
 *   d_out   OUT  f32 [views][size_d][h][w] or NULL: the combined volumes.  A view's part may BE that view's level-0 volume (in
 *                place); no other overlap between any two buffers of the call is allowed
 *   d_nbr   OUT  f32 [views][3][h][w] or NULL: the winners' neighbour state (lo, hi, last) as smx_dev_aggregate_wta_nbr leaves it
 *   d_uq    OUT  f32 [views][3][h][w] or NULL: the second-best state (sec, rest, last) as smx_dev_aggregate_wta_pair_uq leaves it
 * Nothing else is written.  w, h >= 1, w*h < 2^31, 1 <= size_d <= 2^20, |dminl|, |dminr| <= 2^29 (every level's labels stay ints);
 * every volume 4-byte aligned (level 0 and d_out are
 * read and written in 16- or 8-byte units where w and the pointers allow).
 *
 * smx_cscale_combine: host pointers, one view, synchronous.  agg: `scales` host pointers to the levels' volumes; out (the
 * combined volume), best (the winners' costs) and disp_map (dmin + winning slice) may each be NULL. */
#define SMX_CSCALE_MAX_SCALES 5
typedef struct smx_cscale_params { int scales; double lambda; } smx_cscale_params;
void smx_default_cscale_params(smx_cscale_params* p);
int smx_cscale_weights(const smx_cscale_params* p, float* wt);
int smx_cscale_level(int w, int h, int dmin, int size_d, int s, int* w_s, int* h_s, int* dmin_s, int* size_d_s);
int smx_dev_pyr_down(const uint8_t* d_src, uint8_t* d_dst, int w, int h, int channels, void* stream);
int smx_pyr_down(const uint8_t* src, uint8_t* dst, int w, int h, int channels);
int smx_dev_cscale_wta_pair(const smx_cscale_params* p, const float* const* d_agg_l, const float* const* d_agg_r, int w, int h,
                            int dminl, int dminr, int size_d, int64_t* d_keys, float* d_out, float* d_nbr, float* d_uq,
                            void* stream);
int smx_cscale_combine(const smx_cscale_params* p, const float* const* agg, int w, int h, int dmin, int size_d, float* out,
                       float* best, float* disp_map);
/* Test hook, NOT part of the stable contract: the footprint of a workgroup of the pyramid kernel in output pixels. */
int smx_pyr_down_geometry(int* cols, int* rows);
/* Cross-scale aggregation of this context.  NULL switches it off (the default: nothing is allocated or launched).  While it is
 * on, smx_ctx_stereo_pair / _rgb builds the pyramids of both views, aggregates levels 1 .. scales-1 at their own geometry with
 * this context's cost, guide and smx_params, keeps level 0's volumes as when agg_l is requested, and replaces the plain winners
 * by smx_dev_cscale_wta_pair, which overwrites the level-0 volumes with the combined ones.  Everything behind runs unchanged on
 * the combined keys and volumes: best_*, dmap_*, the sub-pixel neighbours, the uniqueness state, LR check, speckle removal, vote,
 * fill, the depth-discontinuity adjustment (it reads the combined left volume) and the weighted median; out->agg_l / agg_r
 * return the combined volumes.  All levels' volumes stay resident: at most 8/7 of the two level-0 volumes.
 * Supported: the guided filter with the gray or the colour guide under the reference, census and AD-Census costs (AD-Census with
 * colour 1 reads the colour pyramid).  The pair call returns SMX_E_ARG with a message for SGM, cross-based aggregation and the
 * scan-line optimiser (their integer volumes and fixed penalties do not rescale across levels), for out->mean_l / mean_r
 * (ambiguous across levels), for a pyramid whose coarsest level is narrower than 2 pixels, and smx_ctx_stereo_pair_async
 * returns it while the setting is on.  The sharded and multi-GPU drivers do not take it.  The levels' contexts and volumes are
 * allocated by the first pair that runs with it on and are released by smx_destroy only: switching it off, or lowering `scales`,
 * keeps them for the next time. */
int smx_ctx_set_cross_scale(smx_ctx* ctx, const smx_cscale_params* p);
/* Test hook, NOT part of the stable contract: the levels above 0 that the context holds for cross-scale and the device bytes of
 * their buffers.  0 and 0 for a context whose pairs never ran with cross-scale on. */
int smx_ctx_cscale_held(const smx_ctx* ctx, int* levels, size_t* bytes);

/* ------------------------------------------------------------------------------------
 * PatchMatch stereo: slanted support windows (Bleyer, Rhemann, Rother, BMVC 2011; not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* Every other matcher here scores one integer label per pixel over a fronto-parallel window.  On a slanted surface that window
 * mixes several disparities: the winner is biased and the sub-pixel fit moves it by at most half a label.  PatchMatch stereo
 * gives each pixel a disparity PLANE (a, b, d0), scores it with the reference's truncated absolute difference plus gradient
 * summed over an adaptive-weight window that lies in the plane, and searches the planes by random initialisation, propagation
 * and refinement.  There is no cost volume: memory does not grow with size_d.  tests/patchmatch_ref.py is this definition in
 * numpy; every output equals it bit for bit, in every run and whatever the launch geometry.
 *
 * Arithmetic.  IEEE f32, every operation rounded on its own in the order written here, nothing contracted; no transcendental,
 * square root or division on the device.  alpha, th_color and th_grad come from smx_params as in the cost volume (oma = 1 -
 * alpha, border = oma * th_color + alpha * th_grad, all f32).
 *
 * Views.  View v (0 left, 1 right) has the labels dmin_v .. dmax_v = dmin_v + size_d - 1; pixel (x, y) with disparity d
 * matches x + d in the other view.  A pixel's state is its plane (a, b, d0) and the plane's cost m.  The plane's disparity at
 * (x + dx, y + dy) is (d0 + a * (float)dx) + b * (float)dy: d0 is the disparity at the pixel itself.
 *
 * Matching cost rho of a tap q = (qx, qy) under disparity d.  I, G: gray and x gradient of the tap's view, Io, Go of the other
 * view, as f32; the gradient is the cost volume's (I[x-1] - I[x+1]) / 2, one-sided at both row ends, and 0 in an image one
 * column wide.  xs = (float)qx + d.  Unless dmin <= d <= dmax and 0 <= xs <= w - 1 (a NaN fails), rho = border.  Otherwise
 * i = floor(xs), t = xs - i, i1 = min(i + 1, w - 1), I' = Io[i] + t * (Io[i1] - Io[i]), G' likewise on Go, and
 * rho = oma * min(|I_q - I'|, th_color) + alpha * min(|G_q - G'|, th_grad), min(v, th) being v < th ? v : th.  For an integer d
 * this is the cell of the reference's cost volume, bit for bit.
 *
 * Plane cost.  m(p, f) = sum over the taps q of the (2 radius + 1)^2 window of tab[|I_p - I_q|] * rho(q, f(q)), with
 * tab[k] = (float)exp(-k / gamma), k = 0 .. 255, computed on the host in double (smx_pm_weights).  Taps outside the image are
 * skipped.  ORDER: one accumulator from +0, rows dy = -radius .. radius, in a row dx = -radius .. radius; each product rounded,
 * then added.
 *
 * Random numbers.  hash(seed, view, pixel, draw) = fmix32(fmix32(fmix32(seed + 0x9E3779B9 * (view + 1)) ^ pixel) ^ draw) with
 * fmix32 the 32-bit finaliser of MurmurHash3 (Appleby): h ^= h >> 16, h *= 0x85EBCA6B, h ^= h >> 13, h *= 0xC2B2AE35,
 * h ^= h >> 16; pixel = y * w + x.  U = (float)(hash >> 8) * 2^-24, in [0, 1).  smx_pm_hash is the host copy.  Draws 0, 1, 2
 * initialise d0, a, b; step k of the refinement of iteration `it` draws 3 + 3 * (32 * it + k) + {0, 1, 2} for d0, a, b.
 *
 * Search.
 *   1. Init, every pixel: d0 = dmin + U * (float)(size_d - 1), a = (2 U - 1) * max_slope, b likewise; m = its cost.
 *   2. For it = 0 .. iterations - 1:
 *      a. Red-black: a pixel's colour is (x + y) & 1.  The pass over colour it & 1 runs first, then the other colour; only
 *         the pixels of the pass's colour change.  The two views do not read each other in a pass.
 *      b. Spatial propagation.  Candidates: the planes of the pixels at (dx, dy) = (-1,0) (1,0) (0,-1) (0,1) (-5,0) (5,0)
 *         (0,-5) (0,5), in this order; all have the other colour.  A candidate (a_n, b_n, d0_n) of neighbour (nx, ny) is
 *         re-centred: d0' = (d0_n + a_n * (float)(x - nx)) + b_n * (float)(y - ny), slopes unchanged.  A neighbour outside the
 *         image gives none, nor does a d0' outside [dmin, dmax].  In order, a candidate whose cost is strictly lower than the
 *         pixel's current cost replaces plane and cost.
 *      c. Refinement.  dd = (float)(size_d - 1) * 0.5, ds = max_slope * 0.5.  While dd >= 0.1: d0' = clamp(d0 + (2 U - 1) * dd,
 *         dmin, dmax), a' = clamp(a + (2 U - 1) * ds, -max_slope, max_slope), b' likewise (clamp(v, lo, hi) = v < lo ? lo : v > hi ?
 *         hi : v, so a zero keeps its sign); adopted if strictly lower; then both halve.  A step perturbs what the step before left.  size_d 1: no step.
 *      d. View propagation, after both colours, left then right, both reading the other view's planes as they were before
 *         either changed: for pixel (x, y) with x' = clamp((int)floor(((float)x + d0) + 0.5), 0, w - 1) the candidate is
 *         (-a', -b', -d0') of the other view's pixel (x', y).  This sign-flipped plane is a simplification of the exact
 *         transform (which re-centres by x - x' - d0' and rescales the slopes by 1 / (1 + a')): the cost test decides.  No
 *         candidate where -d0' lies outside [dmin, dmax]; adopted if strictly lower.
 *   3. Outputs per view: the planes [3][h][w] (a, b, d0), m, disp = d0, label = clamp(floor(d0 + 0.5), dmin, dmax) as f32.
 *
 * Defaults: radius 8, gamma 10, iterations 4, max_slope 2, seed 0 -- a starting point, not measured on real data.  Valid:
 * 0 <= radius <= 17, gamma finite and > 0, 1 <= iterations <= 16, 0 <= max_slope <= 8, w, h >= 1, w < 2^24, w*h < 2^31,
 * 1 <= size_d <= 2^20, |dminl|, |dminr| <= 2^20; anything else is SMX_E_ARG before any device call.
 *
 * smx_dev_patchmatch_pair: device pointers, gray u8 views [h][w]; 3 + 4 * iterations launches and `iterations` device-to-device
 * copies on `stream`; no allocation, no synchronisation (graph-capturable).  Layouts, the left view first:
 *   d_planes OUT f32 [2][3][h][w]     d_cost, d_disp, d_label OUT f32 [2][h][w]
 * Nothing is written outside them and [0, smx_pm_workspace_bytes(w, h)) of d_ws (0 for an invalid w, h); the workspace may hold
 * anything and needs no alignment; a smaller one is SMX_E_WS before any launch.  No two buffers may overlap.
 * smx_dev_pm_plane_cost: the costs m of GIVEN planes of both views (d_planes IN, d_cost OUT), no search, two launches: scores
 * any plane map, such as a ground truth or another matcher's (0, 0, label).  A plane with a NaN or an infinity costs the border
 * constant at the taps where its disparity is not a number in range.
 * smx_patchmatch, smx_pm_plane_cost: host pointers, synchronous. */
typedef struct smx_pm_params { int radius; double gamma; int iterations; double max_slope; uint32_t seed; } smx_pm_params;
void smx_default_pm_params(smx_pm_params* p);
int smx_pm_weights(const smx_pm_params* p, float* tab /* [256] */);
uint32_t smx_pm_hash(uint32_t seed, uint32_t view, uint32_t pixel, uint32_t draw);
size_t smx_pm_workspace_bytes(int w, int h);
int smx_dev_patchmatch_pair(const smx_params* p, const smx_pm_params* pm, const uint8_t* d_left, const uint8_t* d_right, int w,
                            int h, int size_d, int dminl, int dminr, float* d_planes, float* d_cost, float* d_disp,
                            float* d_label, void* d_ws, size_t ws_bytes, void* stream);
int smx_dev_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* d_left, const uint8_t* d_right, int w, int h,
                          int size_d, int dminl, int dminr, const float* d_planes, float* d_cost, void* d_ws, size_t ws_bytes,
                          void* stream);
int smx_patchmatch(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h, int size_d,
                   int dminl, int dminr, float* planes, float* cost, float* disp, float* label);
int smx_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                      int size_d, int dminl, int dminr, const float* planes, float* cost);
/* The fractional filled map of a pair that ran PatchMatch, by the rule of smx_dev_subpixel_pair: d_out = d_disp (the left view's
 * disp) where d_kept -- the LR-checked left map, or the last map of the outlier stages -- passes fill_occlusion's validity
 * test, d_filled elsewhere.  One launch; n floats each; d_out may be none of the inputs. */
int smx_dev_pm_sub_filled(const float* d_disp, const float* d_kept, const float* d_filled, int w, int h, int dminl, float* d_out,
                          void* stream);
/* Test hook, NOT part of the stable contract: the pixels a workgroup of the search kernels takes (columns, rows; in the
 * red-black pass the columns are pixels of one colour). */
int smx_pm_geometry(int* cols, int* rows);
/* PatchMatch stereo of this context.  NULL switches it off (the default: nothing is allocated or launched).  While it is on,
 * smx_ctx_stereo_pair / _rgb (the gray images of the colour pair) runs smx_dev_patchmatch_pair in place of cost, aggregation
 * and winner-take-all: out->dmap_l / dmap_r are the labels and out->best_l / best_r the plane costs.  The LR check and the fill
 * of the reference run on the labels, speckle removal and region voting behind them unchanged.  smx_ctx_patchmatch_maps copies
 * out what the last pair left (SMX_E_ARG if it ran without PatchMatch; any pointer may be NULL): the planes [3][h][w] of either
 * view, sub_l / sub_r = disp, and sub_filled, which follows smx_dev_subpixel_pair's rule: disp where the LR check (and the
 * outlier stages) kept the pixel, the filled label elsewhere.  It is the map for the weighted median, as the sub-pixel fit's
 * filled map is.
 * There is no cost volume, so the stages that read one are refused, and some combinations are deliberately out of scope: the
 * pair call returns SMX_E_ARG with a message for the census and AD-Census costs, colour guidance, SGM, cross-based aggregation,
 * the scan-line optimiser, cross-scale aggregation, the depth-discontinuity adjustment, the uniqueness test, a non-zero
 * smx_ctx_set_subpixel mode and for out->cost_*, agg_* or mean_*; smx_ctx_stereo_pair_async returns it while the setting is on.
 * The sharded and multi-GPU drivers do not take it.  The buffers are allocated by the first pair that runs with it on. */
int smx_ctx_set_patchmatch(smx_ctx* ctx, const smx_pm_params* p);
int smx_ctx_patchmatch_maps(smx_ctx* ctx, float* planes_l, float* planes_r, float* sub_l, float* sub_r, float* sub_filled);
/* Test hook, NOT part of the stable contract: the device bytes the context holds for PatchMatch stereo (planes, disp and
 * workspace).  0 for a context whose pairs never ran with it on. */
int smx_ctx_pm_held(const smx_ctx* ctx, size_t* bytes);

/* ------------------------------------------------------------------------------------
 * The information permeability filter (Cigla, Alatan, Signal Processing: Image Communication 28, 2013; not a stage of the
 * reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* Every other aggregation here has a bounded support.  The permeability filter's support is the whole image at full label
 * resolution, at O(1) per cell: four one-dimensional first-order recurrences per slice (the separable recursive structure of
 * Gastal and Oliveira's domain transform).  A cost reaches a pixel along an L-shaped path with the product of the permeabilities
 * on the way as its weight: a flat surface passes information as far as it extends, a gray or colour edge stops it.
 * tests/perm_ref.py is this definition in numpy; the results equal it bit for bit.
 *
 * Parameters.  sigma: finite and > 0; anything else is SMX_E_ARG before any device call.  The default 32.0 is a starting point
 * chosen on a synthetic textureless band, not measured on real data.
 *
 * Table.  t[k] = (float)exp(-(double)k / sigma), k = 0 .. 255, computed on the host in double (smx_perm_table); t[0] == 1.
 * The kernels hold no transcendental and no floating-point division.
 *
 * Guide.  u8 [h][w][channels], channels 1, 3 or 4, interleaved.  diff of two neighbouring pixels: |dI| for one channel, the
 * maximum of |dI| over R, G, B for 3 or 4 channels (the paper's choice; alpha is ignored).
 *   mu_h[y][x] = t[diff(I[y][x], I[y][x-1])] for x >= 1;   mu_v[y][x] = t[diff(I[y][x], I[y-1][x])] for y >= 1.
 *
 * Per slice C [h][w] of an f32 volume [size_d][h][w], every product and every sum rounded to f32 on its own, no fused
 * multiply-add; NaN, infinities and subnormals as IEEE 754 says.  Along every row:
 *   LR[0] = C[0],      LR[x] = C[x] + mu_h[x] * LR[x-1]     x ascending
 *   RL[w-1] = C[w-1],  RL[x] = C[x] + mu_h[x+1] * RL[x+1]   x descending
 *   Hh[x] = (LR[x] + RL[x]) - C[x]
 * and the same three lines along every column of Hh with mu_v: TB, BT, out = (TB + BT) - Hh.
 *
 * The output is NOT normalised, as in the paper: a pixel's total weight depends on the guide only and is the same for every
 * label, so the winners, the parabola and equiangular sub-pixel fits, the uniqueness ratio and the comparisons of the
 * depth-discontinuity adjustment are what they would be on the normalised volume.  The filtered costs (best_*, agg_*) are
 * weighted SUMS, not means.
 *
 * Winners.  From out by the packed key's rule with the slices ascending: smallest cost, the last slice among equal costs, a NaN
 * never -- the natural-order winner-take-all pass of the aggregations.
 *
 * What it cannot do alone: on hard random texture every permeability is near 0 and a pixel keeps its own cost.  The context
 * therefore runs it BEHIND the guided filter, which supplies the local support; the permeability pass supplies the reach.
 *
 * smx_perm_workspace_bytes: the workspace with which a call on nviews views of size_d slices runs as one chunk whatever its
 * outputs (0 for w, h or size_d < 1, w*h >= 2^31, size_d > 2^20 or nviews not 1 or 2): per view two weight planes, and per slice
 * a scratch plane (LR, then TB) and a plane of the filtered slice, which a call with d_out == NULL keeps there.  A smaller
 * workspace makes the call go in chunks of slices, with the same bits; one that does not hold one slice -- nviews * w * h * 4 *
 * 3 bytes with d_out, * 4 without -- is SMX_E_WS before anything is launched.
 *
 * smx_dev_permeability_wta_pair: on `stream`; no allocation, no synchronisation (graph-capturable); a weight launch, then per
 * chunk the horizontal pass, the vertical pass and the winner-take-all pass.  d_vol_r and d_guide_r may both be NULL for a
 * one-view call (or d_vol_l and d_guide_l).  Outputs as in the other pair entries: with both views the left view's first, the
 * right view's behind it; the one view of a one-view call at the front.
 *   d_out   OUT  f32 [views][size_d][h][w] or NULL: the filtered volumes.  A view's part may BE that view's input volume (in
 *                place); no other overlap between any two buffers of the call is allowed
 *   d_keys  OUT  int64 [views][h][w] or NULL: the packed keys of out (written fresh).  NULL: no winner-take-all pass, and d_nbr
 *                and d_uq must be NULL
 *   d_nbr   OUT  f32 [views][3][h][w] or NULL: the winners' neighbour state as smx_dev_aggregate_wta_nbr leaves it
 *   d_uq    OUT  f32 [views][3][h][w] or NULL: the second-best state as smx_dev_aggregate_wta_pair_uq leaves it
 * Nothing else is written but [0, ws_bytes) of d_ws.  dminl / dminr: the views' first labels (the keys hold slices: they are
 * checked and otherwise unused).  w, h >= 1, w*h < 2^31, 1 <= size_d <= 2^20; volumes and workspace 4-byte aligned.
 * smx_set_max_slices_per_launch of the calling thread bounds the chunk too.
 *
 * smx_permeability_filter: host pointers, one view, synchronous.  out (the filtered volume), best (the winners' costs) and
 * disp_map (dmin + winning slice) may each be NULL. */
typedef struct smx_perm_params { double sigma; } smx_perm_params;
void smx_default_perm_params(smx_perm_params* p);
int smx_perm_table(const smx_perm_params* p, float* t /* [256] */);
size_t smx_perm_workspace_bytes(int w, int h, int size_d, int nviews);
int smx_dev_permeability_wta_pair(const smx_perm_params* p, const float* d_vol_l, const float* d_vol_r, const uint8_t* d_guide_l,
                                  const uint8_t* d_guide_r, int channels, int w, int h, int dminl, int dminr, int size_d,
                                  int64_t* d_keys, float* d_out, float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_permeability_filter(const smx_perm_params* p, const float* volume, const uint8_t* guide, int channels, int w, int h, int dmin,
                            int size_d, float* out, float* best, float* disp_map);
/* The permeability filter of this context.  NULL switches it off (the default: nothing is allocated or launched).  While it is
 * on, smx_ctx_stereo_pair / _rgb keeps the aggregated volumes as when agg_l is requested, runs smx_dev_permeability_wta_pair in
 * place over them and replaces the plain winners.  Everything behind runs unchanged on the new keys and volumes: best_*, dmap_*,
 * the sub-pixel neighbours, the uniqueness state, LR check, speckle removal, vote, fill, the depth-discontinuity adjustment (it
 * reads the filtered left volume) and the weighted median; out->agg_l / agg_r return the filtered volumes.  Guide: the context's
 * gray images, or the colour pair under SMX_GUIDE_RGB.  Supported: the guided filter with either guide under the reference,
 * census and AD-Census costs.  The pair call returns SMX_E_ARG with a message for SGM, cross-based aggregation and the scan-line
 * optimiser (integer [y][x][d] volumes), PatchMatch (no volume), cross-scale aggregation (not built yet) and out->mean_l /
 * mean_r; smx_ctx_stereo_pair_async returns it while the setting is on.  The sharded and multi-GPU drivers do not take it.  The
 * workspace is allocated by the first pair that runs with it on (at most ~1 GiB: the pass goes in chunks of slices). */
int smx_ctx_set_permeability(smx_ctx* ctx, const smx_perm_params* p);
/* Test hook, NOT part of the stable contract: the device bytes the context holds for the permeability filter.  0 for a context
 * whose pairs never ran with it on. */
int smx_ctx_perm_held(const smx_ctx* ctx, size_t* bytes);

/* ------------------------------------------------------------------------------------
 * Non-local cost aggregation on a minimum spanning tree (Yang, CVPR 2012; not a stage of the reference; opt-in)
 * ---------------------------------------------------------------------------------- */

/* The support of a pixel is the whole image, as with the permeability filter, but the weight between two pixels is
 * exp(-dist / sigma) with dist the distance ALONG THE MINIMUM SPANNING TREE of the guide: the path between two pixels is the
 * most similar one that exists, of any shape, where the permeability filter knows L-shaped paths only.  Two sweeps over the
 * tree, leaves to root and root to leaves, give every pixel its exact sum at O(1) per cell.  tests/tree_ref.py is this
 * definition in numpy; the results equal it bit for bit.
 *
 * Parameters.  sigma: finite and > 0; anything else is SMX_E_ARG before any device call.  The default 25.5 is the paper's 0.1 on
 * a [0, 1] scale: a starting point, not measured on real data.
 *
 * Guide.  u8 [h][w][channels], channels 1, 3 or 4, interleaved.  diff of two 4-neighbours as in the permeability filter: |dI|
 * for one channel, the maximum of |dI| over R, G, B for 3 or 4 channels (alpha is ignored).
 *
 * Graph.  Pixel p = y*w + x.  Edge (p, p+1) exists for x < w-1 and has id 2p; edge (p, p+w) exists for y < h-1 and has id 2p+1.
 * The weight of an edge is diff of its two pixels, 0 .. 255.
 *
 * Tree.  Kruskal over the edges in ascending (weight, id) order: an edge joins the tree when its ends are not connected yet.
 * The total order makes the tree unique whatever union-find is used.  Pixel 0 is the root.  The nodes are numbered breadth
 * first; a node's children are visited in ascending pixel index (up, left, right, down), so the children of a node are
 * consecutive numbers and a level is a contiguous run.  `levels` is the number of levels (the root alone is level 0).
 *
 * The blob.  smx_tree_bytes(w, h) bytes, position independent -- it holds indices only -- so it is copied to the device as it
 * is.  n = w*h; every multi-byte value in the host's (little-endian) byte order:
 *   offset 0            u32 n
 *   offset 4            u32 levels
 *   offset 8            u32 order[n]           the pixel index of node i
 *   offset 8 + 4n       u32 parent[n]          the node number of i's parent; 0 for the root
 *   offset 8 + 8n       u32 child_first[n]     the node number of i's first child: the number of nodes that were numbered when i
 *                                              was visited, also where i has no child (so it never decreases, and may be n)
 *   offset 8 + 12n      u32 level_start[n+1]   level l is the nodes level_start[l] .. level_start[l+1]-1; entries 0 .. levels
 *                                              are used (level_start[levels] == n), the rest is 0
 *   offset 12 + 16n     u8  child_count[n]     0 .. 4
 *   offset 12 + 17n     u8  wt[n]              the weight of the edge from i to its parent; 0 for the root
 *   then 0 .. 3 bytes of 0 up to a multiple of 4: smx_tree_bytes(w, h) = (12 + 18n + 3) & ~3.
 * smx_tree_build writes every byte of it, on the host in plain C++ (a counting sort over the 256 weights, a union-find, a
 * queue): deterministic, no device call, about 13 bytes a pixel of temporary host memory.  blob: 4-byte aligned.  smx_tree_bytes
 * is 0 for w or h < 1 or w*h >= 2^31.
 *
 * Tables.  t[k] = (float)exp(-(double)k / sigma) and u[k] = (float)(1.0 - exp(-2.0 * (double)k / sigma)), k = 0 .. 255, computed
 * on the host in double (smx_tree_tables); t[0] == 1, u[0] == 0.  The kernels hold no transcendental and no division.
 *
 * Filter.  Per slice C [h][w] of an f32 volume [size_d][h][w], every product and every sum rounded to f32 on its own, no fused
 * multiply-add; NaN, infinities and subnormals as IEEE 754 says.  With i a node number:
 *   up, the levels descending:   U[i] = C[order[i]];  then for every child c of i, c ascending:  U[i] = U[i] + t[wt[c]] * U[c]
 *   down, the levels ascending:  A[0] = U[0];  A[i] = t[wt[i]] * A[parent[i]] + u[wt[i]] * U[i]
 *   out[order[i]] = A[i]
 * (U[i] is the weighted sum over i's subtree; the second line adds what lies outside it: A[p] - t U[i] seen through the edge,
 * t (A[p] - t U[i]) + U[i].)  A NaN or an infinity anywhere in a slice reaches every pixel of that slice and no other slice.
 *
 * The output is NOT normalised, as in the paper and as with the permeability filter: a pixel's total weight depends on the guide
 * only and is the same for every label, so the winners, the sub-pixel fits, the uniqueness ratio and the comparisons of the
 * depth-discontinuity adjustment are what they would be on the normalised volume.  The filtered costs are weighted SUMS.
 *
 * Winners.  From out by the packed key's rule with the slices ascending, as smx_dev_permeability_wta_pair takes them.
 *
 * smx_tree_workspace_bytes: the workspace with which a call on nviews views of size_d slices runs as one chunk whatever its
 * outputs (0 for w, h or size_d < 1, w*h >= 2^31, size_d > 2^20 or nviews not 1 or 2): per view and slice the breadth-first
 * plane of U and A and a plane of the filtered slice, which a call with d_out == NULL keeps there.  A smaller workspace makes
 * the call go in chunks of slices, with the same bits; one that does not hold one slice -- nviews * w * h * 4 bytes with d_out,
 * twice that without -- is SMX_E_WS before anything is launched.
 *
 * smx_dev_tree_wta_pair: on `stream`; no allocation, no synchronisation (graph-capturable); per chunk one filter launch -- a
 * workgroup per (slice, view), which walks the levels with a workgroup barrier a level -- and the winner-take-all pass.
 * d_tree_l / d_tree_r: the views' blobs on the device, 4-byte aligned, built from the views' guides at this w and h; they are
 * read only.  The call cannot check them: a blob of another shape gives wrong numbers (the kernel skips every index past the
 * tree, so it never leaves the buffers of the call).  d_vol_r and d_tree_r may both be NULL for a one-view call (or d_vol_l and
 * d_tree_l).  d_out, d_keys, d_nbr, d_uq, dminl, dminr, the limits and the alignment as in smx_dev_permeability_wta_pair; d_out
 * may be the input volumes (in place).  smx_set_max_slices_per_launch of the calling thread bounds the chunk too.
 *
 * smx_tree_filter: host pointers, one view, synchronous; it builds the tree itself.  out (the filtered volume), best (the
 * winners' costs) and disp_map (dmin + winning slice) may each be NULL. */
typedef struct smx_tree_params { double sigma; } smx_tree_params;
void smx_default_tree_params(smx_tree_params* p);
size_t smx_tree_bytes(int w, int h);
int smx_tree_build(const uint8_t* guide, int channels, int w, int h, void* blob);
int smx_tree_tables(const smx_tree_params* p, float* t /* [256] */, float* u /* [256] */);
size_t smx_tree_workspace_bytes(int w, int h, int size_d, int nviews);
int smx_dev_tree_wta_pair(const smx_tree_params* p, const float* d_vol_l, const float* d_vol_r, const void* d_tree_l,
                          const void* d_tree_r, int w, int h, int dminl, int dminr, int size_d, int64_t* d_keys, float* d_out,
                          float* d_nbr, float* d_uq, void* d_ws, size_t ws_bytes, void* stream);
int smx_tree_filter(const smx_tree_params* p, const float* volume, const uint8_t* guide, int channels, int w, int h, int dmin,
                    int size_d, float* out, float* best, float* disp_map);
/* The tree filter of this context: a second mode of the permeability filter's place in a pair.  NULL switches it off (the
 * default: nothing is allocated or launched).  While it is on, smx_ctx_stereo_pair / _rgb keeps the aggregated volumes, builds
 * the two trees on the host from the images it was handed -- the gray images, or the colour pair under SMX_GUIDE_RGB --, uploads
 * them and runs smx_dev_tree_wta_pair in place where the permeability pass would run; everything behind runs unchanged, and
 * what is supported and refused is what smx_ctx_set_permeability lists, under this mode's own name.  The two modes exclude each
 * other: smx_ctx_set_tree while the permeability filter is on is SMX_E_ARG, and so is smx_ctx_set_permeability while this mode
 * is on; switch the other off first.  smx_ctx_stereo_pair_async refuses while the mode is on.  The host build costs more than
 * the kernels. */
int smx_ctx_set_tree(smx_ctx* ctx, const smx_tree_params* p);
/* Test hook, NOT part of the stable contract: the device bytes the context holds for the tree filter (workspace and blobs).  0
 * for a context whose pairs never ran with it on. */
int smx_ctx_tree_held(const smx_ctx* ctx, size_t* bytes);

/* Host-side helpers for the packed key (same encoding as the kernels). */
int64_t smx_pack_key(float cost, uint32_t slice);
void smx_unpack_key(int64_t key, float* cost, uint32_t* slice);

/* Per-stage device time (ms) of the calling thread's most recent timed call -- smx_dev_aggregate_wta[_pair]
 * (+ a following smx_dev_finish_pair) or smx_ctx_stereo_pair -- when timing was enabled with smx_set_timing(1):
 * HIP events of the device the call ran on, recorded on its stream at the stage boundaries (the reference prints
 * one wall-clock `duration`, main.cu:52-54,156,184).  smx_stage_times synchronises with the last event.
 *   upload / download: host <-> device copies of smx_ctx_stereo_pair;  guidance: key presets, image planes,
 *   guidance statistics (guidedFilter.cu:58-123);  aggregation: the fused walker (or the multi-kernel passes);
 *   wta: the packed-key pass over the aggregated planes;  finish: decode, LR check, filling (main.cu:112-155).
 * smx_set_timing: 0 off, 1 the times of the LAST call, 2 cumulative over every call since it was switched on
 * (`calls` counts them; up to 32768 stage marks, later ones are counted in `dropped`).  The pipelined entry
 * (smx_ctx_stereo_pair_async) records no stage marks. */
typedef struct smx_stage_ms {
    float upload, guidance, aggregation, wta, finish, download, total;
    int calls;
    int dropped;   /* stage marks that did not fit (mode 2 keeps 32768): > 0 means the sums cover only the first calls */
} smx_stage_ms;
int smx_set_timing(int mode);
int smx_stage_times(smx_stage_ms* out);
/* guidance + aggregation + wta of that call, and its kernel launches */
int smx_last_agg_ms(float* ms, int* launches);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* SMX_H */
