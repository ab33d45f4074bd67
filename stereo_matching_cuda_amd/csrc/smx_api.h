// smx_api.h -- what smx_capi.hip (the thread's state, the device entries, the checks), smx_host.hip (the host-pointer wrappers)
// and smx_ctx.hip (the persistent context) share.  The thread's state itself stays inside smx_capi.hip.
#pragma once
#include "smx_agg.h"
#include "smx_cscale_host.h"
#include "smx_ctx_plan.h"
#include "smx_perm_host.h"
#include "smx_tree_host.h"

namespace smx {

// RAII device allocation of the host-pointer wrappers and of the context.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    // Holds at least `want` bytes afterwards; does nothing where it does already.  A failure leaves it empty: a later call retries.
    hipError_t ensure(size_t want) {
        if (p && bytes >= want) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        const hipError_t e = hipMalloc(&p, want ? want : 1);
        bytes = e == hipSuccess ? want : 0;
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    // allocate and copy up; copy down
    hipError_t upload(const void* host, size_t n) {
        const hipError_t e = ensure(n);
        return e != hipSuccess ? e : hipMemcpy(p, host, n, hipMemcpyHostToDevice);
    }
    hipError_t download(void* host, size_t n) const { return hipMemcpy(host, p, n, hipMemcpyDeviceToHost); }
    template <class T> T* as() { return (T*)p; }
};

// Every aggregation of the C-ABI meets the calling thread's knobs here.  accumulates: the call adds to keys that an earlier
// chunk of the same pair wrote, so the thread's keys_fresh does not apply to it.
int run_aggregation(const AggCall& c, int forced, bool accumulates);
int thread_max_chunk();                // smx_set_max_slices_per_launch of the calling thread
int thread_agg_path();                  // smx_set_agg_path of the calling thread (what smx_create copies)
int agg_status_error(unsigned status);  // a workspace's status word [0] -> SMX_OK or the "hand-off wait ... timed out" error
struct TimingPause { int saved; TimingPause(); ~TimingPause(); };   // while one lives, stage_mark records nothing
bool subpix_mode_ok(int mode);
bool wmf_params_ok(const smx_wmf_params* p);
// (the shape limits, shape_ok and the *_SHAPES texts: smx_ctx_plan.h)
bool census_params_ok(const smx_census_params* p);
constexpr const char* CENSUS_RANGES = "census needs 1 <= rx <= 4, 1 <= ry <= 3, th >= 1";
bool zncc_params_ok(const smx_zncc_params* p);
constexpr const char* ZNCC_RANGES = "ZNCC needs 1 <= rx <= 4 and 1 <= ry <= 4";
bool adcensus_params_ok(const smx_adcensus_params* p);
constexpr const char* ADCENSUS_RANGES = "needs a valid census window, 0 < lambda <= 1e6, 2^-20 <= scale <= 2^20 and colour 0 or 1";
bool speckle_params_ok(const smx_speckle_params* p);
constexpr const char* SPECKLE_RANGES = "needs max_size >= 0 and a finite max_diff >= 0";
bool uniq_ratio_ok(float ratio);
bool sgm_params_ok(const smx_sgm_params* p);
constexpr const char* SGM_RANGES = "needs 0 <= p1 <= p2 <= 4095 and paths 4 or 8";
bool bp_params_ok(const smx_bp_params* p);
constexpr const char* BP_RANGES = "needs 0 <= step, trunc <= 4095, 0 <= iterations <= 64, 1 <= levels <= 8 and a finite data_scale > 0";
bool scanline_params_ok(const smx_scanline_params* p);
constexpr const char* SCANLINE_RANGES = "needs 0 <= p1 <= p2 <= 4095, 1 <= tau_so <= 256 and paths 4 or 8";
bool cross_params_ok(const smx_cross_params* p);       // (smx_cross.hip, beside the limits of its kernels)
constexpr const char* CROSS_RANGES = "needs 1 <= l1 <= 63, 0 <= l2 <= l1, 1 <= tau2 <= tau1 <= 256 and 1 <= iterations <= 4";
bool vote_params_ok(const smx_vote_params* p);         // (smx_vote.hip, beside the limits of its kernels)
constexpr const char* VOTE_RANGES = "needs tau_s >= 0, 0 <= tau_h_pct <= 99, 0 <= iterations <= 8 and interpolate 0 or 1";
bool adjust_params_ok(const smx_adjust_params* p);     // (smx_adjust.hip, beside the limits of its kernel)
constexpr const char* ADJUST_RANGES = "needs 1 <= tau_e <= 512, vertical 0 or 1 and 1 <= iterations <= 8";
constexpr const char* CSCALE_RANGES = "needs 1 <= scales <= 5 and a finite lambda >= 0";
bool pm_params_ok(const smx_pm_params* p);             // (smx_patchmatch.hip, beside the limits of its kernels)
constexpr const char* PM_RANGES = "needs 0 <= radius <= 17, a finite gamma > 0, 1 <= iterations <= 16 and 0 <= max_slope <= 8";
constexpr const char* PERM_RANGES = "needs a finite sigma > 0";
constexpr const char* TREE_RANGES = "needs a finite sigma > 0";
size_t pick_ws_bytes(int w, int h, int size_d);   // workspace of ONE view for the host-pointer entries (smx_host.hip)

}  // namespace smx
