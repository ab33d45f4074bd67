// Internal helpers shared by the HIP translation units of libsmx_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>

#include "smx.h"

namespace smx {

int fail(int code, const char* fmt, ...);

#define SMX_HIP(call)                                                                   \
    do {                                                                                \
        hipError_t e__ = (call);                                                        \
        if (e__ != hipSuccess)                                                          \
            return ::smx::fail(SMX_E_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, \
                               hipGetErrorString(e__));                                 \
    } while (0)

#define SMX_ARG(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) return ::smx::fail(SMX_E_ARG, "%s: bad argument: %s", __func__, #cond); \
    } while (0)

// Float constants derived from smx_params exactly as the reference kernels derive them from the
// macros (costVolume.cu:169-171,184): all in f32, each operation rounded on its own.
struct CostConst {
    float alpha;      // 1.0f*ALPHA
    float oma;        // 1.0f - alpha
    float th_color;   // 1.0f*TH_color
    float th_grad;    // 1.0f*TH_grad
    float border;     // (1 - alpha)*th_color + 1.0f*alpha*th_grad
};

inline CostConst make_cost_const(const smx_params* p) {
    CostConst c;
    c.alpha = 1.0f * p->alpha;
    c.oma = 1.0f - c.alpha;
    c.th_color = 1.0f * p->th_color;
    c.th_grad = 1.0f * p->th_grad;
    float a = c.oma * c.th_color;
    float b = 1.0f * c.alpha * c.th_grad;
    c.border = a + b;
    return c;
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A kernel's dynamic-LDS limit, raised ONCE per device to the most its launcher ever asks for (hipFuncSetAttribute is a
// per-device setting and a runtime call: it does not belong in front of every launch).  One static instance per kernel.
struct LdsLimitOnce {
    std::once_flag done[64];
    hipError_t err[64];
    hipError_t ensure(const void* fn, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const int i = dev & 63;
        std::call_once(done[i], [&] { err[i] = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); });
        return err[i];
    }
};
// Stage boundary of the calling thread's timed call (smx_set_timing(1) / smx_stage_times): records a HIP event of the
// CURRENT device on `st`; a no-op when timing is off.  Stage ids: smx_capi.hip.
enum StageId { ST_BEGIN = 0, ST_UPLOAD, ST_GUIDANCE, ST_WALK, ST_WTA, ST_FINISH, ST_DOWNLOAD, ST_COUNT };
void stage_mark(int stage, hipStream_t st);

// ---- the counter-based hash of PatchMatch stereo's draws and of the MI cost's random start (smx_pm_hash) ----------------
// MurmurHash3's 32-bit finaliser (Appleby); the counter (seed, view, pixel, draw) goes in one word at a time
__host__ __device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__host__ __device__ inline uint32_t pm_hash(uint32_t seed, uint32_t view, uint32_t pix, uint32_t draw) {
    uint32_t h = fmix32(seed + 0x9E3779B9u * (view + 1u));
    h = fmix32(h ^ pix);
    return fmix32(h ^ draw);
}

// ---- packed WTA key ---------------------------------------------------------------------
// key = sord(cost) << 32 | (0xFFFFFFFF - slice), compared as SIGNED 64-bit integers: sord = monotone
// f32 -> i32 (-0 folded to +0), so that the per-pixel reduction of the shards is a plain int64 MIN
// (RCCL ncclInt64 / torch.int64) with no re-encoding.  Smallest key = smallest cost, and among equal
// costs the LARGEST slice: the reference's `best >= q` rule with ascending slices.
// A NaN cost (only from degenerate parameters, e.g. var + eps == 0) never wins, like the reference's
// `best >= q`, which is false for NaN: it maps to the identity key INT64_MAX.
constexpr int64_t KEY_IDENTITY = 0x7FFFFFFFFFFFFFFFll;
__host__ __device__ inline int64_t pack_key(float cost, uint32_t slice) {
    if (cost != cost) return KEY_IDENTITY;
    if (cost == 0.0f) cost = 0.0f;
    uint32_t u = __builtin_bit_cast(uint32_t, cost);
    u = (u & 0x80000000u) ? (~u ^ 0x80000000u) : u;      // negative floats: reverse their order
    return (int64_t)(((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - slice));
}

// The winner of a run of ASCENDING slices in the float domain: smallest cost, among equal costs (-0 == +0) the LAST slice, a NaN
// never -- `take = q <= m` from m = +inf with no slice yet.  That is the order of the packed keys restricted to ascending
// slices; key() packs the winner once (the identity if nothing was taken), and the caller merges it with the key a pixel already
// holds by the integer min.  (Packing every candidate costs ten vector instructions per element, a step costs three.)
struct WtaRun {
    float m = __builtin_inff();
    uint32_t z = 0xFFFFFFFFu;
    __host__ __device__ inline void step(float q, uint32_t slice) {
        const bool take = q <= m;
        m = take ? q : m;
        z = take ? slice : z;
    }
    __host__ __device__ inline int64_t key() const { return z == 0xFFFFFFFFu ? KEY_IDENTITY : pack_key(m, z); }
};

__host__ __device__ inline void unpack_key(int64_t key, float* cost, uint32_t* slice) {
    uint32_t u = (uint32_t)((uint64_t)key >> 32);
    u = (u & 0x80000000u) ? ~(u ^ 0x80000000u) : u;
    *cost = __builtin_bit_cast(float, u);
    *slice = 0xFFFFFFFFu - (uint32_t)((uint64_t)key & 0xFFFFFFFFu);
}

// ---- neighbours of the winner (sub-pixel refinement, smx_subpix.hip) -------------------------------------------------
// WtaRun plus the q of the winner's neighbouring slices: lo = the slice just before the winner, hi = the slice just after it
// (NaN while that slice has not been seen), prev = the previous slice (the run starts it at the pixel's `last`, or at NaN
// for a pixel without a winner yet).  Same winner as WtaRun.
struct WtaRunNbr {
    float m = __builtin_inff();
    uint32_t z = 0xFFFFFFFFu;
    float lo = __builtin_nanf(""), hi = __builtin_nanf(""), prev;
    __host__ __device__ explicit WtaRunNbr(float prev0) : prev(prev0) {}
    __host__ __device__ inline void step(float q, uint32_t slice) {
        const bool take = q <= m;
        const float h1 = z + 1u == slice ? q : hi;      // (no winner yet: z + 1 wraps to 0, and hi means nothing)
        lo = take ? prev : lo;
        hi = take ? __builtin_nanf("") : h1;
        m = take ? q : m;
        z = take ? slice : z;
        prev = q;
    }
    __host__ __device__ inline int64_t key() const { return z == 0xFFFFFFFFu ? KEY_IDENTITY : pack_key(m, z); }
};

// Per-pixel neighbour state d_nbr of a view: three f32 planes [3][h][w] -- 0 lo, 1 hi, 2 last (the q of the last slice
// the view has aggregated).  The merge of a pass's run (slices slice0 .., first q `q0`) with the pixel's incoming key:
// the run wins -> lo, hi of the run; the old winner stays -> lo unchanged, hi = q0 if the winner is slice0 - 1; a key
// that stays the identity has no winner (lo = hi = NaN); always last = the run's prev.  Returns the merged key.
__host__ __device__ inline float nbr_prev0(int64_t key_in, float last_in) { return key_in != KEY_IDENTITY ? last_in : __builtin_nanf(""); }
__host__ __device__ inline int64_t nbr_merge(const WtaRunNbr& r, int64_t key_in, uint32_t slice0, float q0, float* lo, float* hi,
                                             float* last) {
    const int64_t kk = r.key();
    const uint32_t zin = 0xFFFFFFFFu - (uint32_t)((uint64_t)key_in & 0xFFFFFFFFu);
    if (kk < key_in) {
        *lo = r.lo;
        *hi = r.hi;
    } else if (key_in == KEY_IDENTITY) {
        *lo = *hi = __builtin_nanf("");
    } else if (zin + 1u == slice0) {
        *hi = q0;
    }
    *last = r.prev;
    return kk < key_in ? kk : key_in;
}

// ---- second-best cost of the winner (uniqueness test, smx_uniq.hip) ----------------------------------------------------
// WtaRun plus sec = the smallest cost among the seen slices at least two away from the winner (+inf if there is none; a
// NaN never counts), kept in one pass by two more values: rest = the smallest cost of all seen slices but the last seen
// (+inf if none), last = the cost of the last seen slice (NaN if none).  When the winner moves to slice z, every slice up
// to z - 2 is non-adjacent to it, and their minimum is `rest`; while it stays, a slice from z* + 2 on competes for sec
// directly.  Same winner as WtaRun.  Every minimum takes a value only where it is strictly smaller, so among equal costs
// (-0 == +0) the first seen stays: one ascending scan from +inf over the eligible slices gives the same bits.
// The state (m, z, sec, rest, last) is all a run needs: a run resumed from it equals one run over all slices, whatever the
// chunking -- no merge step.  Per-pixel state d_uq of a view: three f32 planes [3][h][w] -- 0 sec, 1 rest, 2 last; m and z
// come back from the pixel's key (resume), an identity key starts blank.
struct WtaRunUq {
    float m = __builtin_inff();
    uint32_t z = 0xFFFFFFFFu;
    float sec = __builtin_inff(), rest = __builtin_inff(), last = __builtin_nanf("");
    __host__ __device__ inline void resume(int64_t key, float sec_in, float rest_in, float last_in) {
        const bool on = key != KEY_IDENTITY;
        float c;
        uint32_t s;
        unpack_key(key, &c, &s);
        m = on ? c : __builtin_inff();
        z = on ? s : 0xFFFFFFFFu;
        sec = on ? sec_in : __builtin_inff();
        rest = on ? rest_in : __builtin_inff();
        last = on ? last_in : __builtin_nanf("");
    }
    __host__ __device__ inline void step(float q, uint32_t slice) {
        const bool take = q <= m;
        // (no winner yet: z + 2 wraps to 1, but every q so far was a NaN, this one too -- else it is taken -- and q < sec is false)
        const bool far = slice >= z + 2u && q < sec;
        sec = take ? rest : (far ? q : sec);
        m = take ? q : m;
        z = take ? slice : z;
        rest = last < rest ? last : rest;
        last = q;
    }
    __host__ __device__ inline int64_t key() const { return z == 0xFFFFFFFFu ? KEY_IDENTITY : pack_key(m, z); }
};

// The uniqueness (peak-ratio) test of one pixel: c0 = the cost of its key, s = its sec.  Rejected iff the key is not the
// identity and s - c0 < ratio * |c0| (f32, each operation rounded on its own); an infinite or NaN s rejects nothing, nor
// does ratio == 0.  *margin = s - c0: +inf where s is unknown (+inf or NaN), NaN where the key is the identity.
__host__ __device__ inline bool uniq_rejects(int64_t key, float s, float ratio, float* margin) {
    if (key == KEY_IDENTITY) { *margin = __builtin_nanf(""); return false; }
    float c0;
    uint32_t z;
    unpack_key(key, &c0, &z);
    if (!(s < __builtin_inff())) { *margin = __builtin_inff(); return false; }     // +inf, NaN: unknown
    const float d = s - c0;
    *margin = d;
    const float bound = ratio * fabsf(c0);
    return ratio > 0.0f && d < bound;
}

// The sub-pixel offset of a winner of cost c0 from its neighbours lo, hi (SMX_SUBPIX_PARABOLA / SMX_SUBPIX_EQUIANGULAR;
// smx_subpixel_delta is the host copy of the C-ABI): 0 for an unknown neighbour (NaN) and for a result that is not finite
__host__ __device__ inline float subpixel_delta(int mode, float c0, float lo, float hi) {
    if (lo != lo || hi != hi) return 0.0f;
    const float a = lo - c0, b = hi - c0;
    const float den = mode == SMX_SUBPIX_PARABOLA ? a + b : fmaxf(a, b);
    const float d = (a - b) / (2.0f * den);
    return d - d == 0.0f ? d : 0.0f;
}

}  // namespace smx
