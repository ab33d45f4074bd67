// smx_ctx_plan.h -- what the persistent context's settings mean for a pair: which opt-in stages run together, what a pair needs
// and which requests it refuses.  Host-only (include/smx.h and the standard library), so that tests/host_ctx_plan_check.cpp
// walks the whole rule set without a GPU.  A new stage is one row of STAGES.
#pragma once
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include "smx.h"

namespace smx {

// ---- shape limits: one predicate, and the maxima of size_d beside it for the kernels' files and the rows below ----------------
constexpr int VOTE_MAX_D = 512, ADJ_MAX_D = 512, WIDE_MAX_D = 1 << 20;     // (the vote's histogram and the adjustment's costs in LDS)
constexpr int CGF_MAX_H = 65535;                                            // (the bands of a colour-guided launch are a grid.y)
constexpr int PM_MAX_DMIN = 1 << 20;
constexpr bool shape_ok(int w, int h, int size_d, int max_d) {
    return w >= 1 && h >= 1 && (long long)w * h < (1ll << 31) && size_d >= 1 && size_d <= max_d;
}
constexpr bool pm_shape_ok(int w, int h, int size_d, int dminl, int dminr) {
    return shape_ok(w, h, size_d, WIDE_MAX_D) && w < (1 << 24) && dminl >= -PM_MAX_DMIN && dminl <= PM_MAX_DMIN &&
           dminr >= -PM_MAX_DMIN && dminr <= PM_MAX_DMIN;
}
#define SMX_STR_(x) #x
#define SMX_STR(x) SMX_STR_(x)
constexpr const char* PLANE_SHAPES = "needs w, h >= 1 and w*h < 2^31";
constexpr const char* SGM_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= " SMX_STR(SMX_SGM_MAX_D);
constexpr const char* BP_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= " SMX_STR(SMX_BP_MAX_D);
constexpr const char* CGF_SHAPES = "needs w >= 1, 1 <= h <= 65535 and w*h < 2^31";
constexpr const char* VOTE_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= 512";
constexpr const char* ADJUST_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= 512";
constexpr const char* CSCALE_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= 2^20";
constexpr const char* PERM_SHAPES = "needs w, h >= 1, w*h < 2^31 and 1 <= size_d <= 2^20";
constexpr const char* PM_SHAPES = "needs w, h >= 1, w < 2^24, w*h < 2^31, 1 <= size_d <= 2^20 and |dminl|, |dminr| <= 2^20";

// ---- the settings: the opt-in state of a context (the setters of include/smx.h write it, nothing else does) --------------------
struct CtxSettings {
    int cost_mode = SMX_COST_REFERENCE;     // smx_ctx_set_cost
    smx_census_params census;
    bool adcensus = false;                  // smx_ctx_set_adcensus: it takes the place of the census cost in every flow
    smx_adcensus_params adc;
    smx_mi_params mi;                       // smx_ctx_set_mi: cost_mode SMX_COST_MI, the third value, which only that setter writes
    smx_zncc_params zncc = {3, 3};          // smx_ctx_set_zncc: cost_mode SMX_COST_ZNCC, the fourth value, likewise
    int agg_mode = SMX_AGG_GUIDED;          // smx_ctx_set_aggregation
    smx_sgm_params sgm;
    int guide_mode = SMX_GUIDE_GRAY;        // smx_ctx_set_guidance
    bool cross = false, so = false, cscale = false, perm = false, bp = false, pm = false, adjust = false, speckle = false, vote = false;
    smx_cross_params cross_params;
    smx_scanline_params so_params;
    smx_cscale_params cs_params;
    smx_perm_params perm_params;
    bool tree = false;                      // smx_ctx_set_tree: the second mode of the permeability filter's row; never on with perm
    smx_tree_params tree_params = {25.5};
    smx_bp_params bp_params;
    smx_pm_params pm_params;
    smx_adjust_params adj_params;
    float uniq = 0.0f;                      // smx_ctx_set_uniqueness: the ratio; 0 = off
    int subpix = 0;                         // smx_ctx_set_subpixel: the fit; 0 = off
    smx_speckle_params spk_params;
    smx_vote_params vote_params;
    smx_cross_params vote_arms;
};

// What one pair asks of the context beyond the eight result planes, decided once per pair by plan_pair.  cost / agg: the whole
// volumes, because the caller wants them or a stage reads them; census: a cost materialised chunk by chunk (the census cost,
// AD-Census, the mutual-information cost, which needs no codes, or the ZNCC cost, whose moments take the codes' place); the rest: the stage runs and its buffers are reserved.  cscale / perm / bp / sgm / so / cross / cgf say where the
// winners come from, pm that PatchMatch takes the place of cost, aggregation and winners.  level: this pair is a level of
// another context's pyramid, which wants its aggregated volumes and nothing behind them (ctx_cscale_levels sets it).
// walker_status: the pair ran the fused aggregation, whose status word the entry reads afterwards.
struct PairPlan {
    bool cost = false, agg = false, subpix = false, census = false, sgm = false, speckle = false, uniq = false, cgf = false,
         cross = false, vote = false, so = false, adjust = false, cscale = false, level = false, pm = false, perm = false, bp = false,
         walker_status = false;
};

// ---- the stage table -----------------------------------------------------------------------------------------------------------
enum CtxStage { S_SGM, S_CGF, S_CROSS, S_SO, S_CSCALE, S_PERM, S_BP, S_PM, S_ADJUST, S_UNIQ, S_SUBPIX, S_SPECKLE, S_VOTE, S_CENSUS,
               S_ADCENSUS, N_STAGES };
constexpr uint32_t bit(int s) { return 1u << s; }
// the aggregations that take the place of the guided filter, and the stages that belong to the guided filter
constexpr uint32_t REPLACING = bit(S_SGM) | bit(S_CROSS) | bit(S_SO) | bit(S_BP) | bit(S_PM);
constexpr uint32_t GUIDED_ONLY = bit(S_CGF) | bit(S_CSCALE) | bit(S_PERM);
enum : unsigned { AT_SETTER = 1, PER_PAIR = 2 };     // where a row's shape limit is checked
enum : unsigned {
    NO_MEAN = 1,        // a pair with the stage on produces no mean images
    READS_COST = 2,     // it reads the whole cost volumes
    READS_AGG = 4,      // it reads the aggregated volumes, so the pair keeps them as if the caller had asked for them
    OWN_AGG = 8,        // its own kernels aggregate in place of the fused walker: no status word to read
};
constexpr int ANY = INT_MAX;

struct StageRow {
    const char* noun;
    const char* setter;
    uint32_t excludes;          // the stages it does not run with (symmetric: see the static_assert)
    unsigned flags;             // NO_MEAN | READS_COST | READS_AGG | OWN_AGG
    struct {
        int max_d, max_h;       // shape_ok(w, h, size_d, max_d) and h <= max_h,
        bool pm_terms;          // and the further terms of pm_shape_ok (w < 2^24, |dmin| <= 2^20)
        const char* shapes;     // that limit in words
        unsigned checked;       // AT_SETTER | PER_PAIR; 0: the stage has no limit of its own
    } limit;
    bool PairPlan::*runs;       // its member of the plan (its buffers in ctx_reserve, its launch in ctx_enqueue)
    const char* why;            // nullptr, or a sentence on what the stage needs of its neighbours, for a conflict's message
};

constexpr StageRow STAGES[N_STAGES] = {
    {"semi-global matching", "smx_ctx_set_aggregation", (REPLACING & ~bit(S_SGM)) | GUIDED_ONLY, NO_MEAN | READS_COST | OWN_AGG,
     {SMX_SGM_MAX_D, ANY, false, SGM_SHAPES, AT_SETTER}, &PairPlan::sgm, nullptr},
    {"colour guidance", "smx_ctx_set_guidance", REPLACING, NO_MEAN | OWN_AGG, {ANY, CGF_MAX_H, false, CGF_SHAPES, PER_PAIR},
     &PairPlan::cgf, nullptr},
    {"cross-based aggregation", "smx_ctx_set_cross", (REPLACING & ~(bit(S_CROSS) | bit(S_SO))) | GUIDED_ONLY, NO_MEAN | OWN_AGG,
     {ANY, ANY, false, PLANE_SHAPES, PER_PAIR}, &PairPlan::cross, nullptr},
    // (alone it reads the whole cost volumes, as SGM does; behind cross-based aggregation it reads that stage's q: plan_pair)
    {"the scan-line optimiser", "smx_ctx_set_scanline", (REPLACING & ~(bit(S_CROSS) | bit(S_SO))) | GUIDED_ONLY,
     NO_MEAN | READS_COST | OWN_AGG, {SMX_SGM_MAX_D, ANY, false, SGM_SHAPES, PER_PAIR}, &PairPlan::so, nullptr},
    {"cross-scale aggregation", "smx_ctx_set_cross_scale", REPLACING | bit(S_PERM), NO_MEAN | READS_AGG,
     {WIDE_MAX_D, ANY, false, CSCALE_SHAPES, PER_PAIR}, &PairPlan::cscale,
     "cross-scale aggregation combines the guided filter's volumes across levels"},
    {"the permeability filter", "smx_ctx_set_permeability", REPLACING | bit(S_CSCALE), NO_MEAN | READS_AGG,
     {WIDE_MAX_D, ANY, false, PERM_SHAPES, PER_PAIR}, &PairPlan::perm,
     "the permeability filter runs over the guided filter's volumes of one scale"},
    {"belief propagation", "smx_ctx_set_bp", (REPLACING & ~bit(S_BP)) | GUIDED_ONLY, NO_MEAN | READS_COST | OWN_AGG,
     {SMX_BP_MAX_D, ANY, false, BP_SHAPES, PER_PAIR}, &PairPlan::bp, nullptr},
    {"PatchMatch stereo", "smx_ctx_set_patchmatch",
     (REPLACING & ~bit(S_PM)) | GUIDED_ONLY | bit(S_CENSUS) | bit(S_ADCENSUS) | bit(S_ADJUST) | bit(S_UNIQ) | bit(S_SUBPIX),
     NO_MEAN | OWN_AGG, {WIDE_MAX_D, ANY, true, PM_SHAPES, AT_SETTER | PER_PAIR}, &PairPlan::pm,
     "PatchMatch stereo keeps no cost volume, and its planes are sub-pixel already"},
    {"the depth-discontinuity adjustment", "smx_ctx_set_adjust", bit(S_PM), READS_AGG,
     {ADJ_MAX_D, ANY, false, ADJUST_SHAPES, AT_SETTER | PER_PAIR}, &PairPlan::adjust, nullptr},
    {"the uniqueness test", "smx_ctx_set_uniqueness", bit(S_PM), 0, {ANY, ANY, false, nullptr, 0}, &PairPlan::uniq, nullptr},
    {"the sub-pixel fit", "smx_ctx_set_subpixel", bit(S_PM), 0, {ANY, ANY, false, nullptr, 0}, &PairPlan::subpix, nullptr},
    {"speckle removal", "smx_ctx_set_speckle", 0, 0, {ANY, ANY, false, PLANE_SHAPES, AT_SETTER}, &PairPlan::speckle, nullptr},
    {"region voting", "smx_ctx_set_vote", 0, 0, {VOTE_MAX_D, ANY, false, VOTE_SHAPES, AT_SETTER}, &PairPlan::vote, nullptr},
    {"the census cost", "smx_ctx_set_cost", bit(S_PM), 0, {ANY, ANY, false, nullptr, 0}, &PairPlan::census, nullptr},
    {"the AD-Census cost", "smx_ctx_set_adcensus", bit(S_PM), 0, {ANY, ANY, false, nullptr, 0}, &PairPlan::census, nullptr},
};

constexpr bool excludes_are_symmetric() {
    for (int a = 0; a < N_STAGES; ++a)
        for (int b = 0; b < N_STAGES; ++b)
            if (((STAGES[a].excludes >> b) & 1) != ((STAGES[b].excludes >> a) & 1) || (a == b && (STAGES[a].excludes >> a) & 1)) return false;
    return true;
}
static_assert(excludes_are_symmetric(), "STAGES: A must list B exactly when B lists A, and no stage lists itself");

// The stages that `s` has on, as bits of CtxStage
inline uint32_t stages_on(const CtxSettings& s) {
    const bool on[N_STAGES] = {s.agg_mode == SMX_AGG_SGM, s.guide_mode == SMX_GUIDE_RGB, s.cross, s.so, s.cscale, s.perm || s.tree, s.bp, s.pm,
                               s.adjust, s.uniq > 0.0f, s.subpix != 0, s.speckle, s.vote, s.cost_mode == SMX_COST_CENSUS || s.cost_mode == SMX_COST_MI || s.cost_mode == SMX_COST_ZNCC,
                               s.adcensus};
    uint32_t m = 0;
    for (int i = 0; i < N_STAGES; ++i) m |= on[i] ? bit(i) : 0;
    return m;
}

// The permeability filter and the tree filter are the two modes of one row and exclude each other at the setters: nullptr where
// the setter of the tree filter (tree) or of the permeability filter (!tree) may switch its mode on under `s`, else the refusal
inline const char* row_mode_conflict(const CtxSettings& s, bool tree) {
    if (tree && s.perm)
        return "smx_ctx_set_tree: the permeability filter is on (smx_ctx_set_permeability): switch it off first, the two do not run together";
    if (!tree && s.tree)
        return "smx_ctx_set_permeability: the tree filter is on (smx_ctx_set_tree): switch it off first, the two do not run together";
    return nullptr;
}

inline bool stage_shape_ok(const StageRow& r, int w, int h, int size_d, int dminl, int dminr) {
    return shape_ok(w, h, size_d, r.limit.max_d) && h <= r.limit.max_h && (!r.limit.pm_terms || pm_shape_ok(w, h, size_d, dminl, dminr));
}

// ---- the plan of one pair ------------------------------------------------------------------------------------------------------
enum PairEntry { ENTRY_GRAY, ENTRY_RGB, ENTRY_ASYNC };
constexpr const char* ENTRY_NAMES[] = {"smx_ctx_stereo_pair", "smx_ctx_stereo_pair_rgb", "smx_ctx_stereo_pair_async"};

// SMX_OK and the plan of a pair of `entry` under the settings `s`, or SMX_E_ARG and in `err` why the pair is refused.  It
// allocates and launches nothing.  channels: 0 on the gray and the pipelined entry.
inline int plan_pair(const CtxSettings& s, int w, int h, int size_d, PairEntry entry, int channels, int dminl, int dminr,
                     bool wants_cost, bool wants_agg, bool wants_mean, PairPlan* plan, char* err, size_t errlen) {
    const char* who = ENTRY_NAMES[entry];
    const uint32_t on = stages_on(s);
    auto is_on = [on](int i) { return (on >> i & 1) != 0; };
    auto refuse = [&](const char* fmt, auto... a) { snprintf(err, errlen, fmt, who, a...); return SMX_E_ARG; };
    // the mutual-information cost and the ZNCC cost are modes of the census cost's row: the same flows and exclusions under
    // their own names
    const bool mi = s.cost_mode == SMX_COST_MI, zncc = s.cost_mode == SMX_COST_ZNCC;
    // and the tree filter is a mode of the permeability filter's row in the same way (the plan's `perm` says that the pass runs,
    // the settings which of the two it is)
    const bool tree = s.tree;
    auto noun = [mi, zncc, tree](int i) {
        return i == S_CENSUS && mi ? "the mutual-information cost" : i == S_CENSUS && zncc ? "the ZNCC cost" : i == S_PERM && tree ? "the tree filter" : STAGES[i].noun;
    };
    auto setter = [mi, zncc, tree](int i) {
        return i == S_CENSUS && mi ? "smx_ctx_set_mi" : i == S_CENSUS && zncc ? "smx_ctx_set_zncc" : i == S_PERM && tree ? "smx_ctx_set_tree" : STAGES[i].setter;
    };
    auto reason = [tree](int i) { return i == S_PERM && tree ? "the tree filter runs over the guided filter's volumes of one scale" : STAGES[i].why; };
    *plan = PairPlan{};
    plan->walker_status = true;
    // the pipelined entry stages the eight planes only: it takes the state with every opt-in off
    for (int i = 0; entry == ENTRY_ASYNC && i < N_STAGES; ++i)
        if (is_on(i)) return refuse("%s: %s is on (%s): use %s", noun(i), setter(i), ENTRY_NAMES[i == S_CGF ? ENTRY_RGB : ENTRY_GRAY]);
    for (int a = 0; a < N_STAGES; ++a)
        for (int b = a + 1; b < N_STAGES; ++b) {
            if (!is_on(a) || !is_on(b) || !(STAGES[a].excludes >> b & 1)) continue;
            const char* why = reason(b) ? reason(b) : reason(a);
            return refuse("%s: %s (%s) and %s (%s) do not run together%s%s", noun(a), setter(a), noun(b), setter(b), why ? ": " : "", why ? why : "");
        }
    if (is_on(S_PM) && (wants_cost || wants_agg))
        return refuse("%s: %s (%s) produces no cost volumes and no aggregated volumes", STAGES[S_PM].noun, STAGES[S_PM].setter);
    if (is_on(S_CGF) && !channels)
        return refuse("%s: %s is on (%s): use %s", STAGES[S_CGF].noun, STAGES[S_CGF].setter, ENTRY_NAMES[ENTRY_RGB]);
    if (is_on(S_ADCENSUS) && s.adc.colour && !channels)
        return refuse("%s: %s takes its AD term from the colour images (%s): use %s", STAGES[S_ADCENSUS].noun, STAGES[S_ADCENSUS].setter,
                      ENTRY_NAMES[ENTRY_RGB]);
    for (int i = 0; i < N_STAGES; ++i) {
        const StageRow& r = STAGES[i];
        if (!is_on(i)) continue;
        if ((r.flags & NO_MEAN) && wants_mean) return refuse("%s: %s (%s) produces no mean images", noun(i), setter(i));
        if ((r.limit.checked & PER_PAIR) && !stage_shape_ok(r, w, h, size_d, dminl, dminr))
            return refuse("%s: %s (%s) %s", noun(i), setter(i), r.limit.shapes);
        plan->*r.runs = true;
        // (behind cross-based aggregation the optimiser reads that stage's q, not the cost volumes)
        plan->cost |= (r.flags & READS_COST) && !(i == S_SO && is_on(S_CROSS));
        plan->agg |= (r.flags & READS_AGG) != 0;
        plan->walker_status &= !(r.flags & OWN_AGG);
    }
    plan->cost |= wants_cost;
    plan->agg |= wants_agg;
    return SMX_OK;
}

}  // namespace smx
