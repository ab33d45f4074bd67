// main.cpp -- drop-in for the reference's entry point (stereo_matching_cuda/main.cu:37-214).
// Same stage order, same progress lines on stdout, same 12 output images, and every stage goes
// through the reference-named host functions of this directory (which forward to the HIP kernels
// behind include/smx.h).  The code itself is organised differently: buffers are std::vectors, the
// options, the refusals and the outputs are table driven, main() is the list of phases, and the image
// normaliser (helpers.cuh) is a two-pass restatement of write_mat.
//
//   smx_main                         reference behaviour: ./data/tsukuba0.png, ./data/tsukuba1.png,
//                                    D_MIN..D_MAX from the macros, outputs into ./data/
//   smx_main L.png R.png [dmin dmax [outdir]] [options]
// options (not in the reference).  The opt-in costs, aggregations and stages (--cost census / adcensus, --aggregation sgm /
// cross / scanline / cross-scanline / patchmatch, --guidance rgb, --uniqueness, --speckle, --vote, --adjust, --subpixel) compose with each other and with --wmf, --pfm and --png16 unless
// an entry says otherwise; none of them goes with --ngpu or --pipeline:
//   --fused           one device-resident call for everything after the gray conversion
//                     (smx_stereo_pair: cost built on the fly inside the fused aggregation) instead of
//                     the reference's stage-by-stage host round trips
//   --host-compare    the reference's self-check mode (main.cu:40 hard-codes it off): every stage also
//                     runs its CPU twin (cpu_twins.cpp) and check_errors() compares exactly
//   --fast            the NON-bit-exact aggregation with wave-parallel row scans (smx_set_agg_path(4); SURVEY 8f rank
//                     4): a few labels differ from the reference's, and on this hardware it is slower than the
//                     exact path -- kept as a measured point, never a default
//   --pfm FILE        filled left disparity (positive pixels) as a Middlebury-style PFM
//   --png16 FILE      filled left disparity as a KITTI-style 16-bit PNG (disparity * 256)
//   --wmf MODE        weighted-median refinement of the filled left map after the fill (smx_weighted_median, default
//                     parameters; Hosni et al.'s last step, not in the reference), on every path: MODE `occluded`
//                     filters the pixels the LR check invalidated, `all` every pixel.  Writes occlu_mapl_wmf.png
//                     beside the 12 images, and --pfm / --png16 then hold the refined map
//   --subpixel FIT    sub-pixel disparity (`parabola` or `equiangular`) from the winners' neighbouring aggregated costs
//                     (smx_ctx_set_subpixel; implies --fused): --pfm / --png16 then hold the sub-pixel filled map.
//                     Not with --wmf
//   --cost census     the census / Hamming matching cost instead of the reference's (smx_ctx_set_cost; implies --fused): the
//                     same twelve images, the two cost images from the census volumes.  --census-window WxH gives the
//                     window in pixels (odd, 3x3 .. 9x7; default 9x7), --census-th N the truncation (>= 1; default 62)
//   --cost adcensus   AD-Census, census plus absolute differences, each through 1 - exp(-c / lambda) (smx_ctx_set_adcensus;
//                     implies --fused): the cost for pairs whose repeating patterns the census cost alone ties on.  The same
//                     twelve images, the two cost images from the AD-Census volumes.  --census-window / --census-th apply to its
//                     census part; --adcensus-lambda C,A gives the two lambda (0 < lambda <= 1e6; default 30,10),
//                     --adcensus-scale S the scale (2^-20 .. 2^20; default 127.5), --ad gray|rgb the images of the absolute
//                     difference: the gray ones (default) or R, G, B of the PNGs (smx_ctx_stereo_pair_rgb).  With
//                     --host-compare the CPU twin (adcensus_costOnCPU) redoes the cost images
//   --cost mi         the mutual-information cost (smx_ctx_set_mi; implies --fused): the cost for pairs whose gray values are
//                     related by some fixed mapping that need not be increasing.  The pair learns a 256 x 256 table from itself:
//                     --mi-iterations N tables (1 .. 16; default 3), from a start map --mi-init random (default; --mi-seed K) or
//                     reference (one pass with the reference's cost).  The same twelve images, the two cost images from the
//                     volumes of the last table.  With --host-compare the table is recomputed from its histogram, the CPU twin
//                     (mi_costOnCPU) redoes the cost images, and the aggregation twins take the last table's volumes.  Not with
//                     --aggregation patchmatch
//   --speckle SIZE[,DIFF]  speckle removal between the LR check and the fill (smx_speckle_filter; not in the reference), on
//                     every single-GPU path: connected components of at most SIZE pixels whose 4-neighbours differ by at
//                     most DIFF (default 1) are invalidated like LR failures.  Writes occlu_mapl_despeckled.png beside
//                     the 12 images; occlu_mapl_filled.png (and --wmf occluded, --subpixel, --pfm, --png16 behind it) then
//                     come from the despeckled map
//   --vote [S,PCT[,N]]  region voting and 16-direction interpolation behind speckle removal (smx_region_vote,
//                     smx_ctx_set_vote; Mei et al.'s outlier refinement, not in the reference), on every single-GPU path: an
//                     invalid pixel takes the most frequent valid label of its cross region if the region holds more than S
//                     valid pixels (default 20) and the label more than PCT percent of them (0 .. 99; default 40), in N rounds
//                     (0 .. 8; default 5); what is left looks along 16 directions (--vote-interpolate 0|1, default 1).  The
//                     value is optional: a word that starts with a digit behind --vote is taken as it.  --vote-arms L1,L2 and
//                     --vote-tau T1,T2 give the support regions (the ranges and defaults of --cross-arms / --cross-tau); their
//                     guide is the left colour image where the pair runs through the colour entry, else the gray one.  Writes
//                     occlu_mapl_voted.png beside the 12 images; occlu_mapl_filled.png (and --wmf, --subpixel, --pfm, --png16
//                     behind it) then come from the voted map, while the validity test of --subpixel and --wmf occluded stays
//                     the one without it.  At most 512 labels.  With --host-compare the CPU twin (region_voteOnCPU) redoes it
//   --adjust [TAU[,N]]  depth-discontinuity adjustment of the filled left map from the left aggregated volume
//                     (smx_ctx_set_adjust; Mei et al.'s step behind the interpolation, not in the reference; implies --fused): a
//                     pixel beside a step of at least TAU labels (1 .. 512; default 2) takes the neighbour's label where the
//                     aggregated volume says that label costs it less, in N rounds (1 .. 8; default 1), so that an edge which the
//                     fill carried across a rejected band moves back by a pixel a round.  The value is optional, like --vote's.
//                     --adjust-vertical 0|1 leaves out or takes the neighbours above and below (default 1).  It runs behind
//                     the fill and --subpixel and in front of --wmf, through every aggregation: occlu_mapl_filled.png, --wmf,
//                     --pfm and --png16 then come from the adjusted map, which occlu_mapl_adjusted.png holds too, and with
//                     --subpixel the changed pixels carry their own fits.  At most 512 labels.  With --host-compare the CPU twin
//                     (discontinuityAdjustOnCPU) redoes it from the twin of the fill
//   --cross-scale [S[,LAMBDA]]  cross-scale cost aggregation for the guided filter (smx_ctx_set_cross_scale; Zhang et al. 2014, not
//                     in the reference; implies --fused): the pair is aggregated at S levels of an image pyramid (1 .. 5; default
//                     4) with the unchanged aggregation, and the winners come from the levels' volumes combined under an
//                     inter-scale regulariser of weight LAMBDA (finite, >= 0; default 1.0).  It helps on textureless surfaces
//                     wider than the filter's window; a coarse label stands for 2^s fine ones, which it cannot split.  The value
//                     is optional, like --vote's.  With the gray or the colour guide and every --cost; the twelve images come
//                     from the combined winners, the two mean images are empty, and disparity_mapl_cscale.png holds the left
//                     map once more.  With --host-compare the CPU twins (pyrDownOnCPU, the cost and guided-filter twins at every
//                     level, crossScaleOnCPU) redo both views and check_errors compares.  Not with --aggregation sgm | cross |
//                     scanline | cross-scanline, --ngpu or --pipeline
//   --permeability [SIGMA]  the information permeability filter behind the guided filter (smx_ctx_set_permeability; Cigla & Alatan
//                     2013, not in the reference; implies --fused): full-image edge-aware aggregation of the aggregated volumes
//                     by four recurrences per slice, with exp(-|dI| / SIGMA) between neighbours (finite, > 0; default 32, a
//                     starting point chosen on a synthetic band, not measured on real data).  The value is optional, like
//                     --vote's.  With the gray or the colour guide and every --cost; the twelve images come from the filtered
//                     winners (their costs are weighted sums, not means), the two mean images are empty, and
//                     disparity_mapl_perm.png holds the left map once more.  With --host-compare the CPU twins (the cost and
//                     guided-filter twins, permeabilityOnCPU) redo both views and check_errors compares.  Not with --aggregation
//                     sgm | cross | scanline | cross-scanline | patchmatch, --cross-scale, --ngpu or --pipeline
//   --aggregation sgm semi-global matching instead of the guided filter (smx_ctx_set_aggregation; implies --fused, and the
//                     census cost, --census-window / --census-th included, unless --cost reference is given): the same
//                     twelve images, the two mean images empty.
//                     --sgm-p P1,P2 gives the penalties (0 <= P1 <= P2 <= 4095; default 10,120), --sgm-paths 4|8 the number
//                     of directions (default 8).  With --host-compare the CPU twin (sgm_aggregateOnCPU) redoes both
//                     views from the cost volumes and check_errors compares.  At most 256 labels
//   --aggregation bp  hierarchical belief propagation instead of the guided filter (smx_ctx_set_bp; Felzenszwalb & Huttenlocher
//                     2006, not in the reference; implies --fused): min-sum message passing on the 4-connected grid with the
//                     smoothness term min(STEP |z - z'|, TRUNC), coarse to fine.  --bp-step STEP and --bp-trunc TRUNC (0 .. 4095;
//                     default 20 and 60), --bp-iterations N per level (0 .. 64; default 5), --bp-levels L (1 .. 8; default 4),
//                     --bp-scale S the factor in front of the clamp of the cost to 0 .. 255 (finite, > 0; default 1).  With every
//                     --cost; the same twelve images, the two mean images empty, and disparity_mapl_bp.png holds the left map
//                     once more.  With --host-compare the CPU twin (beliefPropagationOnCPU) redoes both views from the cost
//                     volumes and check_errors compares the winners and the left volume.  At most 256 labels.  Not with
//                     --guidance rgb, --cross-scale, --permeability, --ngpu or --pipeline
//   --uniqueness PCT  the uniqueness (peak-ratio) test between the LR check and speckle removal (smx_ctx_set_uniqueness; not
//                     in the reference; implies --fused): 0 <= PCT < 100 is OpenCV's uniquenessRatio, i.e. the ratio
//                     PCT / (100 - PCT); 0 is off.  A left pixel whose winner has a non-neighbouring disparity that costs less
//                     than (1 + ratio) times as much is invalidated like an LR failure.  Writes occlu_mapl_unique.png beside
//                     the 12 images; the later stages start from that map.  With --host-compare the CPU twin
//                     (uniqueness_onCPU: brute force over the left aggregated volume) redoes it
//   --guidance rgb    the guided filter with the colour images as its guide instead of the gray ones (smx_ctx_set_guidance,
//                     smx_ctx_stereo_pair_rgb; not in the reference; implies --fused): an edge between two colours of equal
//                     luminance stays an edge.  The same twelve images, the two mean images empty.  With --host-compare the
//                     CPU twin (colour_guided_filterOnCPU) redoes both views from the cost volumes and check_errors
//                     compares.  Not with --aggregation sgm
//   --aggregation cross  cross-based aggregation instead of the guided filter (smx_ctx_set_cross, smx_ctx_stereo_pair_rgb; not in
//                     the reference; implies --fused): colour-adaptive support regions whose guide is the colour pair.  The same
//                     twelve images, the two mean images empty.  --cross-arms L1,L2 gives the arm lengths (1 <= L1 <= 63,
//                     0 <= L2 <= L1; default 34,17), --cross-tau T1,T2 the colour thresholds (1 <= T2 <= T1 <= 256; default
//                     20,6), --cross-iterations N the iterations (1 .. 4; default 4).  With --host-compare the CPU twin
//                     (cross_aggregateOnCPU) redoes both views from the cost volumes and check_errors compares.  Not with
//                     --guidance rgb
//   --aggregation scanline  the scan-line optimiser with colour-adaptive penalties instead of the guided filter
//                     (smx_ctx_set_scanline, smx_ctx_stereo_pair_rgb; Mei et al.'s step between the aggregation and the winners,
//                     not in the reference; implies --fused): semi-global matching whose penalties drop to a quarter where the
//                     step of a path crosses a colour edge of one view and to a tenth where it crosses one in both; the guide is
//                     the colour pair.  --aggregation cross-scanline is Mei's chain: cross-based aggregation (with its --cross-*
//                     options) and then the optimiser on its result, whose four fractional bits are truncated.  The same twelve
//                     images, the two mean images empty.  --so-p P1,P2 gives the penalties (0 <= P1 <= P2 <= 4095; default
//                     127,382, which fit --cost adcensus at its default scale), --so-tau T the colour threshold (1 .. 256; default
//                     15; 256 never lowers a penalty), --so-paths 4|8 the number of directions (default 4).  With --host-compare
//                     the CPU twins (cross_aggregateOnCPU, scanline_optimizeOnCPU) redo both views from the cost volumes and
//                     check_errors compares.  At most 256 labels.  Not with --guidance rgb
//   --aggregation patchmatch  PatchMatch stereo instead of cost volume, aggregation and winner-take-all (smx_ctx_set_patchmatch;
//                     Bleyer et al. 2011, not in the reference; implies --fused): every pixel gets a disparity plane, scored with
//                     the reference's cost over an adaptive-weight window that lies in the plane, so that a slanted surface is
//                     matched as one.  --pm-radius R gives the window (0 .. 17; default 8), --pm-gamma G the colour weight's
//                     scale (> 0; default 10), --pm-iterations N the iterations (1 .. 16; default 4), --pm-slope S the largest
//                     slope (0 .. 8; default 2; 0 is a fronto-parallel search), --pm-seed K the seed (default 0).  The twelve
//                     images come from its labels and plane costs, the two mean images are empty, disparity_mapl_patchmatch.png
//                     holds the fractional left map, and --pfm / --png16 carry the fractional filled map.  --speckle, --vote and
//                     --wmf run behind it on the labels.  With --host-compare the CPU twin (patchMatchOnCPU) redoes both views and
//                     check_errors compares planes, costs, fractional maps and labels.  Not with --cost census | adcensus,
//                     --guidance rgb, --cross-scale, --adjust, --uniqueness, --subpixel, --ngpu or --pipeline
//   --ngpu N          disparity-shard the aggregation over N GPUs of this node: every GPU aggregates
//                     its slice range, ONE RCCL MIN reduce of the packed keys reassembles the map on GPU 0
//                     (the persistent context smx_sharded_create / _run / _destroy of libsmx_rccl.so,
//                     loaded on demand; implies --fused)
//   --overlap         with --ngpu: one aggregation launch per view, the exchange of the left keys runs
//                     under the aggregation of the right volume
//   --pairs K         with --fused / --ngpu: process the pair K times on ONE persistent context (device
//                     buffers, workspace, streams, communicator created once) and print the time per
//                     pair, uploads and downloads included
//   --pipeline        with --fused --pairs K: the K pairs go through the pipelined entry (smx_ctx_stereo_pair_async /
//                     smx_ctx_wait: pinned staging, uploads and downloads under the aggregation of the neighbouring
//                     pairs); the images written are those of the last pair
#include <dlfcn.h>

#include <chrono>
#include <initializer_list>
#include <vector>

#include "adcensus.cuh"
#include "beliefPropagation.cuh"
#include "census.cuh"
#include "colourGuidedFilter.cuh"
#include "costVolume.cuh"
#include "filter.cuh"
#include "guidedFilter.cuh"
#include "helpers.cuh"
#include "mutualInformation.cuh"
#include "occlusion.cuh"
#include "patchMatch.cuh"
#include "permeability.cuh"
#include "png_io.h"
#include "regionVoting.cuh"
#include "rgb_to_grayscale.cuh"
#include "scanlineOptimization.cuh"
#include "crossAggregation.cuh"
#include "crossScale.cuh"
#include "discontinuityAdjustment.cuh"
#include "sgm.cuh"
#include "speckle.cuh"
#include "uniqueness.cuh"
#include "winner_take_all.cuh"
#include "wmf.cuh"

namespace {

// ---- options ------------------------------------------------------------------------------------------------------------------
struct Options {
    std::vector<std::string> positional;
    std::vector<std::string> given;     // the names of the options seen, in order
    bool fused = false, host_compare = false, fast = false;
    std::string pfm, png16;
    std::string wmf;         // "" = no refinement, else "occluded" or "all"
    int subpixel = 0;        // 0 = off, else SMX_SUBPIX_PARABOLA / SMX_SUBPIX_EQUIANGULAR
    bool census = false;     // --cost census
    smx_census_params census_params;
    bool adcensus = false;   // --cost adcensus
    bool ad_rgb = false;     // --ad rgb: the absolute differences on R, G, B of the colour images
    smx_adcensus_params adc_params;     // (its census part is filled from census_params after the parse)
    bool mi = false;         // --cost mi
    smx_mi_params mi_params;
    bool sgm = false;        // --aggregation sgm
    smx_sgm_params sgm_params;
    bool bp = false;         // --aggregation bp
    smx_bp_params bp_params;
    bool cross = false;      // --aggregation cross, and the first stage of cross-scanline
    smx_cross_params cross_params;
    bool so = false;         // --aggregation scanline, and the second stage of cross-scanline
    smx_scanline_params so_params;
    bool speckle = false;    // --speckle
    smx_speckle_params speckle_params;
    bool vote = false;       // --vote
    smx_vote_params vote_params;
    smx_cross_params vote_arms;
    bool adjust = false;     // --adjust
    smx_adjust_params adjust_params;
    bool perm = false;       // --permeability
    smx_perm_params perm_params;
    bool cscale = false;     // --cross-scale
    smx_cscale_params cs_params;
    bool pm = false;         // --aggregation patchmatch
    smx_pm_params pm_params;
    bool rgb = false;        // --guidance rgb
    float uniqueness = 0.0f; // --uniqueness PCT as the ratio PCT / (100 - PCT); 0 = off
    int ngpu = 0;            // 0 = not given: the single-GPU paths
    int pairs = 1;
    bool pipeline = false;
    bool overlap = false;
    bool ok = true;

    bool saw(std::initializer_list<const char*> names) const {
        for (const char* n : names)
            if (std::find(given.begin(), given.end(), n) != given.end()) return true;
        return false;
    }
};

// The value parsers: true if the whole of `v` is a value of the kind.
bool number(const std::string& v, double lo, double hi, double& out) {
    char* end = nullptr;
    out = std::strtod(v.c_str(), &end);
    return !v.empty() && !*end && out >= lo && out <= hi;
}
bool number(const std::string& v, long lo, long hi, long& out) {
    char* end = nullptr;
    out = std::strtol(v.c_str(), &end, 10);
    return !v.empty() && !*end && out >= lo && out <= hi;
}
// A<sep>B; the caller's predicate on a and b follows the call
bool pair_of(const std::string& v, char sep, int& a, int& b) {
    char got = 0, rest = 0;
    return std::sscanf(v.c_str(), "%d%c%d%c", &a, &got, &b, &rest) == 3 && got == sep;
}
bool pair_of(const std::string& v, char sep, double& a, double& b) {
    char got = 0, rest = 0;
    return std::sscanf(v.c_str(), "%lf%c%lf%c", &a, &got, &b, &rest) == 3 && got == sep;
}
// the index of `v` in `words`, or -1
int word(const std::string& v, std::initializer_list<const char*> words) {
    int k = 0;
    for (const char* w : words) {
        if (v == w) return k;
        ++k;
    }
    return -1;
}

struct Switch { const char* name; bool Options::*target; };
const Switch switches[] = {{"--fused", &Options::fused},
                           {"--host-compare", &Options::host_compare},
                           {"--fast", &Options::fast},
                           {"--pipeline", &Options::pipeline},
                           {"--overlap", &Options::overlap}};

// An option with a value: `set` stores it and says whether it is one; if not, "<name> needs <needs>, not `<value>`".
struct ValueOption { const char* name; const char* needs; bool (*set)(const std::string& v, Options& o); };
const ValueOption value_options[] = {
    {"--pfm", "", [](auto& v, auto& o) { o.pfm = v; return true; }},
    {"--png16", "", [](auto& v, auto& o) { o.png16 = v; return true; }},
    {"--ngpu", "", [](auto& v, auto& o) { o.ngpu = std::atoi(v.c_str()); return true; }},
    {"--pairs", "", [](auto& v, auto& o) { o.pairs = std::atoi(v.c_str()); return true; }},
    {"--wmf", "`occluded` or `all`", [](auto& v, auto& o) { o.wmf = v; return word(v, {"occluded", "all"}) >= 0; }},
    {"--subpixel", "`parabola` or `equiangular`", [](auto& v, auto& o) {
         static_assert(SMX_SUBPIX_PARABOLA == 1 && SMX_SUBPIX_EQUIANGULAR == 2, "the modes follow the words");
         o.subpixel = 1 + word(v, {"parabola", "equiangular"});
         return o.subpixel != 0; }},
    {"--cost", "`reference`, `census`, `adcensus` or `mi`", [](auto& v, auto& o) {       // (the last one wins)
         const int k = word(v, {"reference", "census", "adcensus", "mi"});
         o.census = k == 1; o.adcensus = k == 2; o.mi = k == 3;
         return k >= 0; }},
    {"--mi-iterations", "a number of tables N with 1 <= N <= 16", [](auto& v, auto& o) {
         long k = 0;
         const bool good = number(v, 1L, 16L, k);
         o.mi_params.iterations = (int)k;
         return good; }},
    {"--mi-init", "`random` or `reference`", [](auto& v, auto& o) {
         static_assert(SMX_MI_INIT_RANDOM == 0 && SMX_MI_INIT_REFERENCE == 1, "the modes follow the words");
         o.mi_params.init = word(v, {"random", "reference"});
         return o.mi_params.init >= 0; }},
    {"--mi-seed", "a seed K with 0 <= K < 2^32", [](auto& v, auto& o) {
         long k = 0;
         const bool good = number(v, 0L, 4294967295L, k);
         o.mi_params.seed = (uint32_t)k;
         return good; }},
    {"--adcensus-lambda", "C,A with 0 < C, A <= 1e6", [](auto& v, auto& o) {
         double& c = o.adc_params.lambda_census; double& a = o.adc_params.lambda_ad;
         return pair_of(v, ',', c, a) && c > 0 && c <= 1e6 && a > 0 && a <= 1e6; }},
    {"--adcensus-scale", "a scale S with 2^-20 <= S <= 2^20", [](auto& v, auto& o) {
         return number(v, 1.0 / 1048576.0, 1048576.0, o.adc_params.scale); }},
    {"--ad", "`gray` or `rgb`", [](auto& v, auto& o) { const int k = word(v, {"gray", "rgb"}); o.ad_rgb = k == 1; return k >= 0; }},
    {"--census-window", "WxH with odd W in 3 .. 9 and odd H in 3 .. 7", [](auto& v, auto& o) {
         int ww = 0, wh = 0;
         const bool good = pair_of(v, 'x', ww, wh) && ww >= 3 && ww <= 9 && wh >= 3 && wh <= 7 && ww % 2 && wh % 2;
         o.census_params.rx = ww / 2; o.census_params.ry = wh / 2;
         return good; }},
    {"--census-th", "an integer >= 1", [](auto& v, auto& o) {
         long th = 0;
         const bool good = number(v, 1L, 1000000L, th);
         o.census_params.th = (int)th;
         return good; }},
    {"--aggregation", "`guided`, `sgm`, `cross`, `scanline`, `cross-scanline`, `patchmatch` or `bp`", [](auto& v, auto& o) {    // (the last one wins)
         const int k = word(v, {"guided", "sgm", "cross", "scanline", "cross-scanline", "patchmatch", "bp"});
         o.sgm = k == 1; o.cross = k == 2 || k == 4; o.so = k == 3 || k == 4; o.pm = k == 5; o.bp = k == 6;
         return k >= 0; }},
    {"--bp-step", "a step STEP with 0 <= STEP <= 4095", [](auto& v, auto& o) {
         long k = -1;
         const bool good = number(v, 0L, 4095L, k);
         o.bp_params.step = (int)k;
         return good; }},
    {"--bp-trunc", "a truncation TRUNC with 0 <= TRUNC <= 4095", [](auto& v, auto& o) {
         long k = -1;
         const bool good = number(v, 0L, 4095L, k);
         o.bp_params.trunc = (int)k;
         return good; }},
    {"--bp-iterations", "a count N with 0 <= N <= 64", [](auto& v, auto& o) {
         long k = -1;
         const bool good = number(v, 0L, 64L, k);
         o.bp_params.iterations = (int)k;
         return good; }},
    {"--bp-levels", "a count L with 1 <= L <= 8", [](auto& v, auto& o) {
         long k = 0;
         const bool good = number(v, 1L, 8L, k);
         o.bp_params.levels = (int)k;
         return good; }},
    {"--bp-scale", "a finite S > 0", [](auto& v, auto& o) {
         double s = 0.0;
         const bool good = number(v, 0.0, 3.4e38, s) && (float)s > 0.0f;
         o.bp_params.data_scale = (float)s;
         return good; }},
    {"--pm-radius", "a radius R with 0 <= R <= 17", [](auto& v, auto& o) {
         long r = -1;
         const bool good = number(v, 0L, 17L, r);
         o.pm_params.radius = (int)r;
         return good; }},
    {"--pm-gamma", "a finite G > 0", [](auto& v, auto& o) {
         return number(v, 0.0, 1.7976931348623157e308, o.pm_params.gamma) && o.pm_params.gamma > 0.0; }},
    {"--pm-iterations", "a count N with 1 <= N <= 16", [](auto& v, auto& o) {
         long k = 0;
         const bool good = number(v, 1L, 16L, k);
         o.pm_params.iterations = (int)k;
         return good; }},
    {"--pm-slope", "a slope S with 0 <= S <= 8", [](auto& v, auto& o) { return number(v, 0.0, 8.0, o.pm_params.max_slope); }},
    {"--pm-seed", "a seed K with 0 <= K <= 4294967295", [](auto& v, auto& o) {
         long k = -1;
         const bool good = number(v, 0L, 4294967295L, k);
         o.pm_params.seed = (uint32_t)k;
         return good; }},
    {"--so-p", "P1,P2 with 0 <= P1 <= P2 <= 4095", [](auto& v, auto& o) {
         int& p1 = o.so_params.p1; int& p2 = o.so_params.p2;
         return pair_of(v, ',', p1, p2) && p1 >= 0 && p1 <= p2 && p2 <= 4095; }},
    {"--so-tau", "a threshold T with 1 <= T <= 256", [](auto& v, auto& o) {
         long t = 0;
         const bool good = number(v, 1L, 256L, t);
         o.so_params.tau_so = (int)t;
         return good; }},
    {"--so-paths", "4 or 8", [](auto& v, auto& o) {
         const int k = word(v, {"4", "8"});
         o.so_params.paths = k == 1 ? 8 : 4;
         return k >= 0; }},
    {"--cross-arms", "L1,L2 with 1 <= L1 <= 63 and 0 <= L2 <= L1", [](auto& v, auto& o) {
         int& l1 = o.cross_params.l1; int& l2 = o.cross_params.l2;
         return pair_of(v, ',', l1, l2) && l1 >= 1 && l1 <= 63 && l2 >= 0 && l2 <= l1; }},
    {"--cross-tau", "T1,T2 with 1 <= T2 <= T1 <= 256", [](auto& v, auto& o) {
         int& t1 = o.cross_params.tau1; int& t2 = o.cross_params.tau2;
         return pair_of(v, ',', t1, t2) && t2 >= 1 && t2 <= t1 && t1 <= 256; }},
    {"--cross-iterations", "1, 2, 3 or 4", [](auto& v, auto& o) {
         o.cross_params.iterations = 1 + word(v, {"1", "2", "3", "4"});
         return o.cross_params.iterations != 0; }},
    {"--sgm-p", "P1,P2 with 0 <= P1 <= P2 <= 4095", [](auto& v, auto& o) {
         int& p1 = o.sgm_params.p1; int& p2 = o.sgm_params.p2;
         return pair_of(v, ',', p1, p2) && p1 >= 0 && p1 <= p2 && p2 <= 4095; }},
    {"--sgm-paths", "4 or 8", [](auto& v, auto& o) {
         const int k = word(v, {"4", "8"});
         o.sgm_params.paths = k == 0 ? 4 : 8;
         return k >= 0; }},
    {"--speckle", "SIZE[,DIFF] with SIZE >= 0 and a finite DIFF >= 0", [](auto& v, auto& o) {
         int& size = o.speckle_params.max_size; float& diff = o.speckle_params.max_diff;
         char comma = 0, rest = 0;
         size = -1; diff = 1.0f;
         const int got = std::sscanf(v.c_str(), "%d%c%f%c", &size, &comma, &diff, &rest);
         o.speckle = true;
         return (got == 1 || (got == 3 && comma == ',')) && size >= 0 && diff >= 0.0f && diff <= 3.4e38f; }},
    {"--vote-interpolate", "0 or 1", [](auto& v, auto& o) {
         o.vote_params.interpolate = word(v, {"0", "1"});
         return o.vote_params.interpolate >= 0; }},
    {"--vote-arms", "L1,L2 with 1 <= L1 <= 63 and 0 <= L2 <= L1", [](auto& v, auto& o) {
         int& l1 = o.vote_arms.l1; int& l2 = o.vote_arms.l2;
         return pair_of(v, ',', l1, l2) && l1 >= 1 && l1 <= 63 && l2 >= 0 && l2 <= l1; }},
    {"--vote-tau", "T1,T2 with 1 <= T2 <= T1 <= 256", [](auto& v, auto& o) {
         int& t1 = o.vote_arms.tau1; int& t2 = o.vote_arms.tau2;
         return pair_of(v, ',', t1, t2) && t2 >= 1 && t2 <= t1 && t1 <= 256; }},
    {"--adjust-vertical", "0 or 1", [](auto& v, auto& o) {
         o.adjust_params.vertical = word(v, {"0", "1"});
         return o.adjust_params.vertical >= 0; }},
    {"--uniqueness", "a percentage PCT with 0 <= PCT < 100", [](auto& v, auto& o) {
         char* end = nullptr;
         const float pct = std::strtof(v.c_str(), &end);
         o.uniqueness = pct / (100.0f - pct);
         return !v.empty() && !*end && pct >= 0.0f && pct < 100.0f; }},
    {"--guidance", "`gray` or `rgb`", [](auto& v, auto& o) { const int k = word(v, {"gray", "rgb"}); o.rgb = k == 1; return k >= 0; }},
};

// An option whose value may be left out: the next word is its value iff it starts with a digit.  `set` gets "" without one.
const ValueOption optional_value_options[] = {
    {"--vote", "S,PCT[,N] with S >= 0, 0 <= PCT <= 99 and 0 <= N <= 8", [](auto& v, auto& o) {
         smx_vote_params& p = o.vote_params;
         o.vote = true;
         if (v.empty()) return true;
         char c1 = 0, c2 = 0, rest = 0;
         p.tau_s = p.tau_h_pct = -1;
         const int got = std::sscanf(v.c_str(), "%d%c%d%c%d%c", &p.tau_s, &c1, &p.tau_h_pct, &c2, &p.iterations, &rest);
         return ((got == 3 && c1 == ',') || (got == 5 && c1 == ',' && c2 == ',')) && p.tau_s >= 0 && p.tau_h_pct >= 0 &&
                p.tau_h_pct <= 99 && p.iterations >= 0 && p.iterations <= 8; }},
    {"--permeability", "a finite SIGMA > 0", [](auto& v, auto& o) {
         o.perm = true;
         if (v.empty()) return true;
         char rest = 0;
         const int got = std::sscanf(v.c_str(), "%lf%c", &o.perm_params.sigma, &rest);
         return got == 1 && std::isfinite(o.perm_params.sigma) && o.perm_params.sigma > 0.0; }},
    {"--cross-scale", "S[,LAMBDA] with 1 <= S <= 5 and a finite LAMBDA >= 0", [](auto& v, auto& o) {
         smx_cscale_params& p = o.cs_params;
         o.cscale = true;
         if (v.empty()) return true;
         char comma = 0, rest = 0;
         p.scales = 0;
         const int got = std::sscanf(v.c_str(), "%d%c%lf%c", &p.scales, &comma, &p.lambda, &rest);
         return (got == 1 || (got == 3 && comma == ',')) && p.scales >= 1 && p.scales <= SMX_CSCALE_MAX_SCALES &&
                std::isfinite(p.lambda) && p.lambda >= 0.0; }},
    {"--adjust", "TAU[,N] with 1 <= TAU <= 512 and 1 <= N <= 8", [](auto& v, auto& o) {
         smx_adjust_params& p = o.adjust_params;
         o.adjust = true;
         if (v.empty()) return true;
         char comma = 0, rest = 0;
         p.tau_e = 0;
         const int got = std::sscanf(v.c_str(), "%d%c%d%c", &p.tau_e, &comma, &p.iterations, &rest);
         return (got == 1 || (got == 3 && comma == ',')) && p.tau_e >= 1 && p.tau_e <= 512 && p.iterations >= 1 && p.iterations <= 8; }},
};

// A row of a table of refusals: the first row that holds prints its message, and the exit status is 2.
struct Rule { bool refused; std::string message; };

Options parse(int argc, char** argv) {
    Options o;
    smx_default_census_params(&o.census_params);
    smx_default_speckle_params(&o.speckle_params);
    smx_default_sgm_params(&o.sgm_params);
    smx_default_cross_params(&o.cross_params);
    smx_default_scanline_params(&o.so_params);
    smx_default_adcensus_params(&o.adc_params);
    smx_default_mi_params(&o.mi_params);
    smx_default_vote_params(&o.vote_params);
    smx_default_cross_params(&o.vote_arms);
    smx_default_adjust_params(&o.adjust_params);
    smx_default_cscale_params(&o.cs_params);
    smx_default_perm_params(&o.perm_params);
    smx_default_pm_params(&o.pm_params);
    smx_default_bp_params(&o.bp_params);
    auto refuse = [&o](const std::string& message) { std::fprintf(stderr, "%s\n", message.c_str()); o.ok = false; return o; };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a.rfind("--", 0) != 0) { o.positional.push_back(a); continue; }
        o.given.push_back(a);
        const Switch* s = std::find_if(std::begin(switches), std::end(switches), [&](const Switch& row) { return a == row.name; });
        if (s != std::end(switches)) { o.*(s->target) = true; continue; }
        const ValueOption* opt_k = std::find_if(std::begin(optional_value_options), std::end(optional_value_options),
                                                [&](const ValueOption& row) { return a == row.name; });
        if (opt_k != std::end(optional_value_options)) {
            const bool has_value = i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9';
            const std::string v = has_value ? argv[++i] : "";
            if (!opt_k->set(v, o)) return refuse(a + " needs " + opt_k->needs + ", not `" + v + "`");
            continue;
        }
        const ValueOption* k = std::find_if(std::begin(value_options), std::end(value_options),
                                            [&](const ValueOption& row) { return a == row.name; });
        if (k == std::end(value_options)) return refuse("unknown option " + a);
        if (i + 1 >= argc) return refuse(a + " needs a value");
        const std::string v = argv[++i];
        if (!k->set(v, o)) return refuse(a + " needs " + k->needs + ", not `" + v + "`");
    }
    if (o.sgm && !o.saw({"--cost"})) o.census = true;     // census + SGM is the standard pairing
    o.adc_params.census = o.census_params;
    o.adc_params.colour = o.ad_rgb ? 1 : 0;
    // the options that only go with a mode (after the lines above: the census options go with the implied cost too)
    const Rule rules[] = {
        {o.saw({"--census-window", "--census-th"}) && !o.census && !o.adcensus,
         "--census-window and --census-th need the census cost (--cost census, or --aggregation sgm without --cost reference) "
         "or --cost adcensus"},
        {o.saw({"--adcensus-lambda", "--adcensus-scale", "--ad"}) && !o.adcensus,
         "--adcensus-lambda, --adcensus-scale and --ad need --cost adcensus"},
        {o.saw({"--mi-iterations", "--mi-init", "--mi-seed"}) && !o.mi, "--mi-iterations, --mi-init and --mi-seed need --cost mi"},
        {o.mi && o.pm, "--cost mi cannot be combined with --aggregation patchmatch, which scores planes with the reference's cost "
                       "and keeps no cost volume"},
        {o.saw({"--sgm-p", "--sgm-paths"}) && !o.sgm, "--sgm-p and --sgm-paths need --aggregation sgm"},
        {o.saw({"--cross-arms", "--cross-tau", "--cross-iterations"}) && !o.cross,
         "--cross-arms, --cross-tau and --cross-iterations need --aggregation cross or cross-scanline"},
        {o.saw({"--so-p", "--so-tau", "--so-paths"}) && !o.so,
         "--so-p, --so-tau and --so-paths need --aggregation scanline or cross-scanline"},
        {o.saw({"--vote-interpolate", "--vote-arms", "--vote-tau"}) && !o.vote,
         "--vote-interpolate, --vote-arms and --vote-tau need --vote"},
        {o.saw({"--adjust-vertical"}) && !o.adjust, "--adjust-vertical needs --adjust"},
        {o.saw({"--pm-radius", "--pm-gamma", "--pm-iterations", "--pm-slope", "--pm-seed"}) && !o.pm,
         "--pm-radius, --pm-gamma, --pm-iterations, --pm-slope and --pm-seed need --aggregation patchmatch"},
        {o.saw({"--bp-step", "--bp-trunc", "--bp-iterations", "--bp-levels", "--bp-scale"}) && !o.bp,
         "--bp-step, --bp-trunc, --bp-iterations, --bp-levels and --bp-scale need --aggregation bp"},
        {o.perm && (o.sgm || o.cross || o.so || o.pm || o.bp),
         "--permeability runs behind the guided filter: it cannot be combined with --aggregation sgm, cross, scanline, "
         "cross-scanline, patchmatch or bp"},
        {o.perm && o.cscale, "--permeability cannot be combined with --cross-scale"}};
    for (const Rule& r : rules)
        if (r.refused) return refuse(r.message);
    return o;
}

// ---- the pair and what is computed from it -------------------------------------------------------------------------------------
struct Pair {
    int w = 0, h = 0;
    unsigned char* rgb[2] = {nullptr, nullptr};
    int channels[2] = {0, 0};
};

bool load_pair(const std::string& left, const std::string& right, Pair& p) {
    int w2 = 0, h2 = 0;
    p.rgb[0] = smx_png_load(left.c_str(), &p.w, &p.h, &p.channels[0]);
    p.rgb[1] = smx_png_load(right.c_str(), &w2, &h2, &p.channels[1]);
    return p.rgb[0] && p.rgb[1] && p.channels[0] >= 3 && p.channels[1] >= 3 && p.w == w2 && p.h == h2;
}

// What every phase behind the options reads: the images and the label range.
struct Job {
    const Options& opt;
    Pair in;
    unsigned char* gray[2] = {nullptr, nullptr};
    int w = 0, h = 0, n = 0;
    // left volume: labels d_lo .. d_hi; right volume: labels -d_hi .. -d_lo   (main.cu:79-82)
    int d_lo = 0, d_hi = 0, size_d = 0, dmin[2] = {0, 0};
    // --cost mi: the table of the pair's last pass (smx_ctx_mi_table), which every cost volume built afterwards reads
    std::vector<unsigned char> mi_table;
};

// The maps of the pair, as the stages leave them on the host.
struct Maps {
    std::vector<float> best[2], dmap[2], cost[2];
    std::vector<unsigned char> mean[2];
    std::vector<float> occlusion, filled;
    std::vector<float> despeckled;     // --speckle: the LR-checked left map without its small components
    std::vector<float> voted;          // --vote: the last of these maps with its outliers voted on and interpolated
    std::vector<float> perm;           // --permeability: the left map of the filtered winners (= dmap[0])
    std::vector<float> bp;             // --aggregation bp: the left map of its winners (= dmap[0])
    std::vector<float> cscale;         // --cross-scale: the left map of the combined winners (= dmap[0])
    std::vector<float> pm_disp;        // --aggregation patchmatch: the fractional left map (the planes' d0)
    std::vector<float> adjusted;       // --adjust: the filled left map with the pixels beside its depth steps adjusted (= filled)
    std::vector<float> unique;         // --uniqueness: the LR-checked left map without its ambiguous winners
    std::vector<float> sub_filled;     // --subpixel: the sub-pixel filled left map
    std::vector<float> refined;        // --wmf: the weighted median of the filled left map

    explicit Maps(int n) {
        // WTA presets of main.cu:112-118: memset(best, 9999999.0f) stores byte 0x7F everywhere
        for (int v = 0; v < 2; ++v) {
            best[v].resize(n);
            std::memset(best[v].data(), 0x7F, sizeof(float) * n);
            dmap[v].assign(n, 0.0f);
            mean[v].assign(n, 0);
        }
    }
};

// The first `slices` slices of view v's cost volume, by the cost the options name.
void build_cost(const Job& j, int v, int slices, float* dst, bool host_compare) {
    const Options& opt = j.opt;
    if (opt.mi) {
        compute_mi_cost(j.mi_table.data(), j.gray[0], j.gray[1], v, dst, j.w, j.h, slices, j.dmin[v], host_compare);
    } else if (opt.adcensus) {
        // the images of its absolute differences, and their bytes per pixel
        unsigned char* const* img = opt.ad_rgb ? j.in.rgb : j.gray;
        compute_adcensus_cost(img[v], img[1 - v], opt.ad_rgb ? j.in.channels[0] : 1, dst, j.w, j.h, slices, j.dmin[v],
                              opt.adc_params, host_compare);
    } else if (opt.census) {
        compute_census_cost(j.gray[v], j.gray[1 - v], dst, j.w, j.h, slices, j.dmin[v], opt.census_params);
    } else {
        CHECK(smx_compute_cost(&smx_config().params, j.gray[v], j.gray[1 - v], dst, j.w, j.w, j.h, j.h, slices, j.dmin[v]));
    }
}

// --host-compare of --aggregation sgm / cross / scanline / cross-scanline and --guidance rgb: the mode's twin redoes both views from whole cost volumes
// built by the stage wrappers, from the reference's presets.
void check_aggregation_twin(const Job& j, Maps& m, std::vector<float>& agg_l) {
    const Options& opt = j.opt;
    const int n = j.n;
    bool ok = true;
    for (int v = 0; v < 2; ++v) {
        std::vector<float> vol((size_t)n * j.size_d), tb(n), td(n, 0.0f);
        std::memset(tb.data(), 0x7F, sizeof(float) * n);
        build_cost(j, v, j.size_d, vol.data(), false);
        if (opt.sgm)
            sgm_aggregateOnCPU(vol.data(), nullptr, tb.data(), td.data(), j.w, j.h, j.size_d, j.dmin[v], opt.sgm_params);
        else if (opt.bp) {
            // (the left belief too, where the pair fetched it)
            std::vector<float> ta(v == 0 ? agg_l.size() : 0);
            beliefPropagationOnCPU(vol.data(), ta.empty() ? nullptr : ta.data(), tb.data(), td.data(), j.w, j.h, j.size_d, j.dmin[v],
                                   opt.bp_params);
            if (!ta.empty()) ok = check_errors(ta.data(), agg_l.data(), (int)ta.size()) && ok;
        } else if (opt.so) {
            // alone on the cost volume; in the chain on the q of the cross twin, whose own winners are discarded
            std::vector<float> q(opt.cross ? vol.size() : 0), ub(n), ud(n, 0.0f);
            std::memset(ub.data(), 0x7F, sizeof(float) * n);
            if (opt.cross)
                cross_aggregateOnCPU(j.in.rgb[v], j.in.channels[v], vol.data(), ub.data(), ud.data(), q.data(), j.w, j.h, j.size_d,
                                     j.dmin[v], opt.cross_params);
            scanline_optimizeOnCPU(j.in.rgb[v], j.in.rgb[1 - v], j.in.channels[v], opt.cross ? q.data() : vol.data(), nullptr,
                                   tb.data(), td.data(), j.w, j.h, j.size_d, j.dmin[v], opt.so_params);
        } else if (opt.rgb)
            colour_guided_filterOnCPU(j.in.rgb[v], j.in.channels[v], vol.data(), tb.data(), td.data(), nullptr, j.w, j.h,
                                      j.size_d, j.dmin[v], smx_config().params.radius, smx_config().params.eps);
        else
            cross_aggregateOnCPU(j.in.rgb[v], j.in.channels[v], vol.data(), tb.data(), td.data(), nullptr, j.w, j.h, j.size_d,
                                 j.dmin[v], opt.cross_params);
        ok = check_errors(tb.data(), m.best[v].data(), n) && ok;
        ok = check_errors(td.data(), m.dmap[v].data(), n) && ok;
    }
    if (ok)
        std::cout << (opt.sgm ? "Semi-global matching" : opt.bp ? "Belief propagation" : opt.so ? "Scan-line optimisation" : opt.rgb ? "Colour guided filter"
                                                                                                      : "Cross-based aggregation") << " ok!"
                  << std::endl;
}

// --host-compare of --permeability: per view the cost of the options and the guided-filter twin slice by slice (from the preset,
// a slice's filtered cost is its aggregated plane) or the colour-guided twin, then the permeability twin on the context's guide;
// its winners against the pair's, and the left filtered volume against the context's where that was fetched.
void check_permeability_twin(const Job& j, Maps& m, std::vector<float>& agg_l) {
    const Options& opt = j.opt;
    const int ch = j.in.channels[0];
    const size_t n = (size_t)j.n;
    bool ok = true;
    for (int v = 0; v < 2; ++v) {
        std::vector<float> cost(n * j.size_d), vol(n * j.size_d), tb(n), td(n);
        std::vector<unsigned char> mean(n);
        build_cost(j, v, j.size_d, cost.data(), false);
        if (opt.rgb) {
            std::memset(tb.data(), 0x7F, sizeof(float) * n);
            colour_guided_filterOnCPU(j.in.rgb[v], ch, cost.data(), tb.data(), td.data(), vol.data(), j.w, j.h, j.size_d, j.dmin[v],
                                      smx_config().params.radius, smx_config().params.eps);
        } else {
            std::memset(vol.data(), 0x7F, sizeof(float) * vol.size());
            for (int z = 0; z < j.size_d; ++z)
                guided_filter_onCpu(j.gray[v], cost.data() + z * n, vol.data() + z * n, td.data(), mean.data(), j.w, j.h, 1,
                                    j.dmin[v] + z);
        }
        std::vector<float> out(n * j.size_d), best(n), disp(n);
        permeabilityOnCPU(vol.data(), opt.rgb ? j.in.rgb[v] : j.gray[v], opt.rgb ? ch : 1, out.data(), best.data(), disp.data(), j.w,
                          j.h, j.dmin[v], j.size_d, opt.perm_params);
        // the winners through the reference's presets, as the pair's finish takes them
        std::fill(td.begin(), td.end(), 0.0f);
        std::memset(tb.data(), 0x7F, sizeof(float) * n);
        for (size_t i = 0; i < n; ++i)
            if (tb[i] >= best[i]) { tb[i] = best[i]; td[i] = disp[i]; }
        ok = check_errors(tb.data(), m.best[v].data(), j.n) && ok;
        ok = check_errors(td.data(), m.dmap[v].data(), j.n) && ok;
        if (v == 0 && !agg_l.empty()) {
            for (size_t i = 0; i < out.size(); ++i)
                if (std::memcmp(&out[i], &agg_l[i], 4) != 0 && !(out[i] != out[i] && agg_l[i] != agg_l[i])) {
                    std::cout << "error at element " << i << " of the filtered left volume" << std::endl;
                    ok = false;
                    break;
                }
        }
    }
    if (ok) std::cout << "Permeability ok!" << std::endl;
}

// --host-compare of --cross-scale: per view and level the pyramid twin, the cost of the options at the level's geometry and the
// guided-filter twin slice by slice (from the preset, a slice's filtered cost is its aggregated plane), then the combination twin;
// its winners against the pair's, and the left combined volume against the context's where that was fetched.
void check_cross_scale_twin(const Job& j, Maps& m, std::vector<float>& agg_l) {
    const Options& opt = j.opt;
    const int S = opt.cs_params.scales;
    const bool colour = opt.rgb || opt.ad_rgb;
    const int ch = j.in.channels[0];
    // the pyramids: level 0 is the pair itself
    std::vector<std::vector<unsigned char>> gray[2], rgb[2];
    std::vector<Job> level(S, Job{opt});
    for (int s = 0; s < S; ++s) {
        Job& l = level[s];
        int size_l, size_r;
        smx_cscale_level(j.w, j.h, j.dmin[0], j.size_d, s, &l.w, &l.h, &l.dmin[0], &size_l);
        smx_cscale_level(j.w, j.h, j.dmin[1], j.size_d, s, &l.w, &l.h, &l.dmin[1], &size_r);
        l.n = l.w * l.h;
        l.in.w = l.w; l.in.h = l.h;
        for (int v = 0; v < 2; ++v) {
            l.in.channels[v] = j.in.channels[v];
            l.mi_table = j.mi_table;        // (the levels take the table of level 0)
            if (s == 0) { l.gray[v] = j.gray[v]; l.in.rgb[v] = j.in.rgb[v]; continue; }
            const Job& b = level[s - 1];
            gray[v].emplace_back((size_t)l.n);
            pyrDownOnCPU(b.gray[v], gray[v].back().data(), b.w, b.h, 1);
            l.gray[v] = gray[v].back().data();
            if (colour) {
                rgb[v].emplace_back((size_t)l.n * ch);
                pyrDownOnCPU(b.in.rgb[v], rgb[v].back().data(), b.w, b.h, ch);
                l.in.rgb[v] = rgb[v].back().data();
            }
        }
    }
    bool ok = true;
    for (int v = 0; v < 2; ++v) {
        std::vector<std::vector<float>> vols(S);
        const float* ptrs[SMX_CSCALE_MAX_SCALES] = {};
        for (int s = 0; s < S; ++s) {
            Job& l = level[s];
            int ws, hs, lo;
            smx_cscale_level(j.w, j.h, j.dmin[v], j.size_d, s, &ws, &hs, &lo, &l.size_d);
            const size_t n = (size_t)l.n;
            std::vector<float> cost(n * l.size_d), tb(n), td(n);
            std::vector<unsigned char> mean(n);
            vols[s].resize(n * l.size_d);
            if (opt.adcensus && opt.ad_rgb) {
                // (the stage wrapper makes the gray images of the census codes from the colour images it is given; a level's gray
                // image is the pyramid of the gray image, so the cost twin takes both pyramids here)
                std::vector<float> table(SMX_ADCENSUS_TABLE_FLOATS);
                CHECK(smx_adcensus_tables(&opt.adc_params, table.data()));
                adcensus_costOnCPU(l.in.rgb[v], l.in.rgb[1 - v], l.gray[v], l.gray[1 - v], ch, cost.data(), l.w, l.h, l.size_d,
                                   l.dmin[v], opt.adc_params, table.data());
            } else {
                build_cost(l, v, l.size_d, cost.data(), false);
            }
            if (opt.rgb) {
                std::memset(tb.data(), 0x7F, sizeof(float) * n);
                colour_guided_filterOnCPU(l.in.rgb[v], ch, cost.data(), tb.data(), td.data(), vols[s].data(), l.w, l.h, l.size_d,
                                          l.dmin[v], smx_config().params.radius, smx_config().params.eps);
            } else {
                std::memset(vols[s].data(), 0x7F, sizeof(float) * vols[s].size());
                for (int z = 0; z < l.size_d; ++z)
                    guided_filter_onCpu(l.gray[v], cost.data() + z * n, vols[s].data() + z * n, td.data(), mean.data(), l.w, l.h, 1,
                                        l.dmin[v] + z);
            }
            ptrs[s] = vols[s].data();
        }
        const size_t n = (size_t)j.n;
        std::vector<float> out(n * j.size_d), best(n), disp(n), tb(n), td(n, 0.0f);
        crossScaleOnCPU(ptrs, out.data(), best.data(), disp.data(), j.w, j.h, j.dmin[v], j.size_d, opt.cs_params);
        // the winners through the reference's presets, as the pair's finish takes them
        std::memset(tb.data(), 0x7F, sizeof(float) * n);
        for (size_t i = 0; i < n; ++i)
            if (tb[i] >= best[i]) { tb[i] = best[i]; td[i] = disp[i]; }
        ok = check_errors(tb.data(), m.best[v].data(), j.n) && ok;
        ok = check_errors(td.data(), m.dmap[v].data(), j.n) && ok;
        if (v == 0 && !agg_l.empty()) {
            for (size_t i = 0; i < out.size(); ++i)
                if (std::memcmp(&out[i], &agg_l[i], 4) != 0 && !(out[i] != out[i] && agg_l[i] != agg_l[i])) {
                    std::cout << "error at element " << i << " of the combined left volume" << std::endl;
                    ok = false;
                    break;
                }
        }
    }
    if (ok) std::cout << "Cross-scale ok!" << std::endl;
}

// --host-compare of --aggregation patchmatch: the twin redoes the search of both views; its planes, plane costs, fractional maps
// and labels against the context's.
void check_patchmatch_twin(const Job& j, Maps& m, std::vector<float>& planes, std::vector<float>& disp) {
    const size_t n = (size_t)j.n;
    std::vector<float> tp(6 * n), tc(2 * n), td(2 * n), tl(2 * n);
    patchMatchOnCPU(j.gray[0], j.gray[1], tp.data(), tc.data(), td.data(), tl.data(), j.w, j.h, j.size_d, j.dmin[0], j.dmin[1],
                    j.opt.pm_params);
    bool ok = check_errors(tp.data(), planes.data(), (int)(6 * n));
    ok = check_errors(td.data(), disp.data(), (int)(2 * n)) && ok;
    for (int v = 0; v < 2; ++v) {
        ok = check_errors(tc.data() + v * n, m.best[v].data(), j.n) && ok;
        ok = check_errors(tl.data() + v * n, m.dmap[v].data(), j.n) && ok;
    }
    if (ok) std::cout << "PatchMatch ok!" << std::endl;
}

// --host-compare of the device-resident flow behind the winners: LR check, uniqueness (from the left aggregated volume), speckle
// removal, region voting, fill and depth-discontinuity adjustment, each twin from the twin before it.
void check_finish_twins(const Job& j, Maps& m, std::vector<float>& agg_l) {
    const Options& opt = j.opt;
    const int n = j.n;
    const float vmin = (float)j.d_lo, invalid = (float)(j.d_lo - 100);
    std::vector<float> lr(m.dmap[0]);
    detect_occlusionOnCPU(lr.data(), m.dmap[1].data(), j.dmin[0] - 100, j.w, j.h);
    bool ok = check_errors(lr.data(), m.occlusion.data(), n);
    if (opt.uniqueness > 0.0f) {
        std::vector<float> twin(n);
        uniqueness_onCPU(agg_l.data(), lr.data(), twin.data(), nullptr, j.w, j.h, j.size_d, opt.uniqueness, vmin, invalid);
        const bool same = check_errors(twin.data(), m.unique.data(), n);
        if (same) std::cout << "Uniqueness ok!" << std::endl;
        ok = same && ok;
        lr = twin;
    }
    if (opt.speckle) {
        std::vector<float> twin(n);
        speckle_filterOnCPU(lr.data(), twin.data(), j.w, j.h, vmin, invalid, opt.speckle_params);
        ok = check_errors(twin.data(), m.despeckled.data(), n) && ok;
        lr = twin;
    }
    if (opt.vote) {
        // (the guide of the context: the left colour image where the pair ran through the colour entry)
        const bool colour = opt.rgb || opt.ad_rgb || opt.cross || opt.so;
        std::vector<float> twin(n);
        region_voteOnCPU(colour ? j.in.rgb[0] : j.gray[0], colour ? j.in.channels[0] : 1, lr.data(), m.dmap[1].data(), twin.data(),
                         j.w, j.h, j.d_lo, j.size_d, opt.vote_params, opt.vote_arms);
        const bool same = check_errors(twin.data(), m.voted.data(), n);
        if (same) std::cout << "Region voting ok!" << std::endl;
        ok = same && ok;
        lr = twin;
    }
    fill_occlusionOnCPU(lr.data(), j.w, j.h, vmin);
    if (opt.adjust) {
        // (the context hands out the adjusted map only: the twin of the fill goes through the twin of the adjustment)
        std::vector<float> twin(n);
        discontinuityAdjustOnCPU(lr.data(), agg_l.data(), twin.data(), j.w, j.h, j.d_lo, j.size_d, opt.adjust_params, 0, nullptr);
        lr = twin;
    }
    const bool same_filled = check_errors(lr.data(), m.filled.data(), n);
    if (opt.adjust && same_filled) std::cout << "Discontinuity adjustment ok!" << std::endl;
    ok = same_filled && ok;
    if (ok) std::cout << "Occlusion ok!" << std::endl;
}

// ---- the two flows ----------------------------------------------------------------------------------------------------------------
// The reference's data flow: every stage is a host -> device -> host round trip.
void run_stage_by_stage(const Job& j, Maps& m) {
    const Options& opt = j.opt;
    const bool host_compare = opt.host_compare;
    const int w = j.w, h = j.h, n = j.n;
    for (int v = 0; v < 2; ++v) m.cost[v].resize((size_t)n * j.size_d);
    std::cout << "Cost Volume ..." << std::endl;
    for (int v = 0; v < 2; ++v) compute_cost(j.gray[v], j.gray[1 - v], m.cost[v].data(), w, w, h, h, j.dmin[v], host_compare);
    std::cout << "guided filter ..." << std::endl;
    for (int v = 0; v < 2; ++v)
        compute_guided_filter(j.gray[v], m.cost[v].data(), m.best[v].data(), m.dmap[v].data(), m.mean[v].data(), w, h, j.size_d,
                              j.dmin[v], host_compare);
    std::cout << "guided filter ok" << std::endl;
    // left-right check on a copy of the left map, then scan-line filling on a copy of that
    std::vector<unsigned char> unused_u8[2] = {std::vector<unsigned char>(n, 0), std::vector<unsigned char>(n, 0)};
    m.occlusion = m.dmap[0];
    detect_occlusion(m.occlusion.data(), m.dmap[1].data(), j.dmin[0] - 100, unused_u8[0].data(), unused_u8[1].data(), w,
                     h);                                                                 // main.cu:149-150
    if (opt.speckle) {
        m.despeckled.resize(n);
        speckle_filter(m.occlusion.data(), m.despeckled.data(), w, h, (float)j.d_lo, (float)(j.d_lo - 100), opt.speckle_params,
                       host_compare);
    }
    m.filled = opt.speckle ? m.despeckled : m.occlusion;
    if (opt.vote) {
        m.voted.resize(n);
        region_vote(j.gray[0], 1, m.filled.data(), m.dmap[1].data(), m.voted.data(), w, h, j.d_lo, j.size_d, opt.vote_params,
                    opt.vote_arms, host_compare);
        m.filled = m.voted;
    }
    fill_occlusion(m.filled.data(), w, h, (float)j.d_lo);                                // main.cu:154-155
}

// The multi-GPU driver (RCCL) is loaded only when asked for, so the plain binary does not need librccl.
struct Sharded {
    int (*create)(const smx_params*, int, int, int, int, int, void**) = nullptr;
    int (*run)(void*, const uint8_t*, const uint8_t*, int, int, const smx_pair_out*) = nullptr;
    int (*destroy)(void*) = nullptr;

    bool load() {
        void* so = dlopen("libsmx_rccl.so", RTLD_NOW | RTLD_LOCAL);
        create = so ? (decltype(create))dlsym(so, "smx_sharded_create") : nullptr;
        run = so ? (decltype(run))dlsym(so, "smx_sharded_run") : nullptr;
        destroy = so ? (decltype(destroy))dlsym(so, "smx_sharded_destroy") : nullptr;
        return create && run && destroy;
    }
};

// Device-resident: one call, the cost slices never leave the CU (only slice 0 of each volume is materialised, for the two cost
// images the reference writes).  -> whether `stage_ms` holds the device times of the last pair.
bool run_device_resident(Job& j, const Sharded& sh, Maps& m, smx_stage_ms& stage_ms) {
    const Options& opt = j.opt;
    const bool host_compare = opt.host_compare, uniq = opt.uniqueness > 0.0f;
    const bool colour = opt.rgb || opt.ad_rgb || opt.cross || opt.so;     // the entry that takes the colour pair
    const int w = j.w, h = j.h, n = j.n;
    std::cout << "Cost Volume ..." << std::endl;
    for (int v = 0; v < 2; ++v) m.cost[v].resize((size_t)n);
    // (the mutual-information cost has its table only behind the pair: its cost images follow the pair below)
    for (int v = 0; v < 2 && !opt.mi; ++v) build_cost(j, v, 1, m.cost[v].data(), host_compare);
    std::cout << "guided filter ..." << std::endl;
    m.occlusion.resize(n);
    m.filled.resize(n);
    smx_pair_out out;
    std::memset(&out, 0, sizeof(out));
    out.best_l = m.best[0].data(); out.best_r = m.best[1].data();
    out.dmap_l = m.dmap[0].data(); out.dmap_r = m.dmap[1].data();
    // (SGM, the colour guide, cross-based aggregation, the scan-line optimiser, cross-scale, the permeability filter and PatchMatch have no
    // mean images)
    if (!opt.sgm && !opt.bp && !opt.rgb && !opt.cross && !opt.so && !opt.cscale && !opt.pm && !opt.perm) { out.mean_l = m.mean[0].data(); out.mean_r = m.mean[1].data(); }
    out.occlusion = m.occlusion.data(); out.filled = m.filled.data();
    std::vector<float> agg_l;          // the left aggregated volume: what the uniqueness and adjustment twins read
    if ((uniq || opt.adjust || opt.cscale || opt.perm || opt.bp) && host_compare) {
        agg_l.resize((size_t)n * j.size_d);
        out.agg_l = agg_l.data();
    }
    // one persistent context for all pairs: nothing is allocated, created or destroyed per pair
    void* sctx = nullptr;
    smx_ctx* ctx = nullptr;
    if (sh.create) CHECK(sh.create(&smx_config().params, w, h, j.size_d, opt.ngpu, opt.overlap ? 1 : 0, &sctx));
    else CHECK(smx_create(&smx_config().params, w, h, j.size_d, &ctx));
    if (opt.subpixel) CHECK(smx_ctx_set_subpixel(ctx, opt.subpixel));
    if (opt.census) CHECK(smx_ctx_set_cost(ctx, SMX_COST_CENSUS, &opt.census_params));
    if (opt.adcensus) CHECK(smx_ctx_set_adcensus(ctx, &opt.adc_params));
    if (opt.mi) CHECK(smx_ctx_set_mi(ctx, &opt.mi_params));
    if (opt.speckle) CHECK(smx_ctx_set_speckle(ctx, &opt.speckle_params));
    if (uniq) CHECK(smx_ctx_set_uniqueness(ctx, opt.uniqueness));
    if (opt.vote) CHECK(smx_ctx_set_vote(ctx, &opt.vote_params, &opt.vote_arms));
    if (opt.adjust) CHECK(smx_ctx_set_adjust(ctx, &opt.adjust_params));
    if (opt.cscale) CHECK(smx_ctx_set_cross_scale(ctx, &opt.cs_params));
    if (opt.perm) CHECK(smx_ctx_set_permeability(ctx, &opt.perm_params));
    if (opt.sgm) CHECK(smx_ctx_set_aggregation(ctx, SMX_AGG_SGM, &opt.sgm_params));
    if (opt.bp) CHECK(smx_ctx_set_bp(ctx, &opt.bp_params));
    if (opt.rgb) CHECK(smx_ctx_set_guidance(ctx, SMX_GUIDE_RGB));
    if (opt.cross) CHECK(smx_ctx_set_cross(ctx, &opt.cross_params));      // (its guide: the colour pair)
    if (opt.so) CHECK(smx_ctx_set_scanline(ctx, &opt.so_params));         // (behind the cross stage where that is on too)
    if (opt.pm) CHECK(smx_ctx_set_patchmatch(ctx, &opt.pm_params));
    if (!sh.create) CHECK(smx_set_timing(1));     // per-stage device times of the last pair (smx_stage_times)
    auto run_pair = [&]() {
        return sh.create ? sh.run(sctx, j.gray[0], j.gray[1], j.dmin[0], j.dmin[1], &out)
               : colour  ? smx_ctx_stereo_pair_rgb(ctx, j.in.rgb[0], j.in.rgb[1], j.in.channels[0], j.dmin[0], j.dmin[1], &out)
                         : smx_ctx_stereo_pair(ctx, j.gray[0], j.gray[1], j.dmin[0], j.dmin[1], &out);
    };
    CHECK(run_pair());
    if (opt.pairs > 1) {
        const bool pipelined = opt.pipeline && !sh.create;
        const auto t0 = std::chrono::steady_clock::now();
        if (pipelined) {
            // two pairs in flight; every result is copied out of the staging into the same output buffers
            for (int k = 1; k < opt.pairs; ++k) {
                CHECK(smx_ctx_stereo_pair_async(ctx, j.gray[0], j.gray[1], j.dmin[0], j.dmin[1]));
                if (k >= 2) CHECK(smx_ctx_wait(ctx, nullptr, &out));
            }
            CHECK(smx_ctx_wait(ctx, nullptr, &out));
        } else {
            for (int k = 1; k < opt.pairs; ++k) CHECK(run_pair());
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("pairs %d on one context: %.3f ms per pair, uploads and downloads included%s\n", opt.pairs - 1,
                    ms / (opt.pairs - 1), pipelined ? " (pipelined entry)" : "");
    }
    bool have_stage_ms = false;
    if (!sh.create) {
        have_stage_ms = smx_stage_times(&stage_ms) == SMX_OK;
        CHECK(smx_set_timing(0));
    }
    if (opt.subpixel) {
        m.sub_filled.resize(n);
        CHECK(smx_ctx_subpixel_maps(ctx, nullptr, nullptr, m.sub_filled.data()));
    }
    if (opt.speckle) {
        m.despeckled.resize(n);
        CHECK(smx_ctx_speckle_map(ctx, m.despeckled.data()));
    }
    if (opt.vote) {
        m.voted.resize(n);
        CHECK(smx_ctx_vote_map(ctx, m.voted.data()));
    }
    if (uniq) {
        m.unique.resize(n);
        CHECK(smx_ctx_uniqueness_map(ctx, m.unique.data(), nullptr));
    }
    if (opt.mi) {
        // the table the last pass ran with, and the histogram it came from: the twin of the table is the library's own host
        // arithmetic, so --host-compare checks that the two belong together
        j.mi_table.resize((size_t)SMX_MI_LEVELS * SMX_MI_LEVELS);
        std::vector<uint32_t> hist(j.mi_table.size());
        CHECK(smx_ctx_mi_table(ctx, j.mi_table.data(), hist.data()));
        if (host_compare) {
            std::vector<unsigned char> again(j.mi_table.size());
            CHECK(smx_mi_table(hist.data(), again.data()));
            if (again == j.mi_table) std::cout << "Mutual-information table ok!" << std::endl;
            else std::cout << "error in the mutual-information table" << std::endl;
        }
        for (int v = 0; v < 2; ++v) build_cost(j, v, 1, m.cost[v].data(), host_compare);
    }
    if (opt.adjust) m.adjusted = m.filled;
    if (opt.cscale) m.cscale = m.dmap[0];
    if (opt.perm) m.perm = m.dmap[0];
    if (opt.bp) m.bp = m.dmap[0];
    std::vector<float> pm_planes, pm_disp;      // both views' planes and fractional maps: what the twin is compared with
    if (opt.pm) {
        pm_planes.resize((size_t)6 * n);
        pm_disp.resize((size_t)2 * n);
        m.sub_filled.resize(n);
        CHECK(smx_ctx_patchmatch_maps(ctx, pm_planes.data(), pm_planes.data() + (size_t)3 * n, pm_disp.data(), pm_disp.data() + n,
                                      m.sub_filled.data()));
        m.pm_disp.assign(pm_disp.begin(), pm_disp.begin() + n);
    }
    if (sh.create) CHECK(sh.destroy(sctx));
    else CHECK(smx_destroy(ctx));
    std::cout << "guided filter ok" << std::endl;
    // (with --cross-scale the winners are the combination's: its twin redoes the colour guide's aggregation at every level)
    // (and with --permeability the filter's: its twin redoes the aggregation of either guide in front of it)
    if (host_compare && opt.perm) check_permeability_twin(j, m, agg_l);
    else if (host_compare && opt.cscale) check_cross_scale_twin(j, m, agg_l);
    else if (host_compare && (opt.sgm || opt.bp || opt.rgb || opt.cross || opt.so)) check_aggregation_twin(j, m, agg_l);
    else if (host_compare && opt.pm) check_patchmatch_twin(j, m, pm_planes, pm_disp);
    if (host_compare) check_finish_twins(j, m, agg_l);
    return have_stage_ms;
}

// ---- the files ----------------------------------------------------------------------------------------------------------------------
// The 12 images of the reference, then the maps of the opt-in stages that ran.  -> the number of files that could not be written.
int write_outputs(const Job& j, const Maps& m, const std::string& outdir) {
    const Options& opt = j.opt;
    const int w = j.w, h = j.h, n = j.n;
    struct U8Out { const char* name; const unsigned char* data; };
    struct F32Out { const char* name; const std::vector<float>& data; };      // written if not empty
    const U8Out u8_outputs[] = {{"image_left.png", j.gray[0]}, {"image_right.png", j.gray[1]},
                                {"image_mean_left.png", m.mean[0].data()},
                                {"image_mean_right.png", m.mean[1].data()}};
    // file names of the reference (its cost images are named after its default range)
    const F32Out f32_outputs[] = {{"best_costl.png", m.best[0]},       {"best_costr.png", m.best[1]},
                                  {"cost_lminus15.png", m.cost[0]},    {"cost_rminus15.png", m.cost[1]},
                                  {"occlu_mapl.png", m.occlusion},     {"disparity_mapl.png", m.dmap[0]},
                                  {"disparity_mapr.png", m.dmap[1]},   {"occlu_mapl_filled.png", m.filled},
                                  {"occlu_mapl_despeckled.png", m.despeckled}, {"occlu_mapl_unique.png", m.unique},
                                  {"occlu_mapl_voted.png", m.voted}, {"occlu_mapl_adjusted.png", m.adjusted},
                                  {"disparity_mapl_cscale.png", m.cscale},
                                  {"disparity_mapl_perm.png", m.perm},
                                  {"disparity_mapl_bp.png", m.bp},
                                  {"disparity_mapl_patchmatch.png", m.pm_disp},
                                  {"occlu_mapl_wmf.png", m.refined}};
    int write_failures = 0;
    for (const U8Out& o : u8_outputs)
        if (!smx_png_write((outdir + "/" + o.name).c_str(), w, h, 1, o.data)) ++write_failures;
    for (const F32Out& o : f32_outputs) {
        if (o.data.empty()) continue;
        const std::vector<unsigned char> img = normalise_like_reference(o.data.data(), (size_t)n);
        if (!smx_png_write((outdir + "/" + o.name).c_str(), w, h, 1, img.data())) ++write_failures;
    }
    // disparity outputs in dataset conventions: positive pixel offsets of the filled left map (the refined one with --wmf,
    // the sub-pixel one with --subpixel)
    const std::vector<float>& final_map = !m.sub_filled.empty() ? m.sub_filled : m.refined.empty() ? m.filled : m.refined;
    if (!opt.pfm.empty()) {
        std::vector<float> d(n);
        for (int i = 0; i < n; ++i) d[i] = -final_map[i];
        if (!smx_pfm_write(opt.pfm.c_str(), w, h, d.data())) ++write_failures;
    }
    if (!opt.png16.empty()) {
        std::vector<unsigned short> d(n);
        for (int i = 0; i < n; ++i) {
            const float v = -final_map[i] * 256.0f;
            d[i] = (unsigned short)(v < 0.0f ? 0.0f : (v > 65535.0f ? 65535.0f : v));
        }
        if (!smx_png_write_gray16(opt.png16.c_str(), w, h, d.data())) ++write_failures;
    }
    return write_failures;
}

}  // namespace

int main(int argc, char** argv) {
    // ---- options and refusals
    const Options opt = parse(argc, argv);
    if (!opt.ok) return 2;
    const bool host_compare = opt.host_compare;   // main.cu:40 (the reference hard-codes false)
    std::printf("Starting...\n");
    if (smx_device_count() < 1) {
        std::fprintf(stderr, "no HIP device available\n");
        return 1;
    }
    std::printf("Using Device %d: %s\n", 0, smx_version());
    if (opt.fast && smx_set_agg_path(4) != SMX_OK) {
        std::fprintf(stderr, "--fast: %s\n", smx_last_error());
        return 1;
    }

    std::string left = "./data/tsukuba0.png", right = "./data/tsukuba1.png", outdir = "./data";
    const std::vector<std::string>& pos = opt.positional;
    if (pos.size() >= 2) { left = pos[0]; right = pos[1]; }
    if (pos.size() >= 4) { smx_config().d_min = std::atoi(pos[2].c_str()); smx_config().d_max = std::atoi(pos[3].c_str()); }
    if (pos.size() >= 5) outdir = pos[4];
    Job job{opt};
    const int d_lo = job.d_lo = smx_config().d_min, d_hi = job.d_hi = smx_config().d_max;
    const long long labels = (long long)d_hi - d_lo + 1;
    if (d_hi < d_lo || labels > 4096) {
        std::fprintf(stderr, "bad disparity range [%d, %d]: need dmin <= dmax and at most 4096 labels\n", d_lo, d_hi);
        return 2;
    }
    job.size_d = (int)labels;
    job.dmin[0] = d_lo;
    job.dmin[1] = -d_hi;
    // What does not compose.  The first row that holds decides which option the message names (SGM stands before the census
    // cost it implies: the message names the option that was given).
    const bool uniq = opt.uniqueness > 0.0f;
    const bool multi = opt.ngpu != 0 || opt.pipeline;
    const std::string with_multi = " cannot be combined with --ngpu or --pipeline";
    const Rule refusals[] = {
        {opt.subpixel && (!opt.wmf.empty() || multi),
         "--subpixel cannot be combined with --wmf (the median works on integer labels), --ngpu or --pipeline"},
        {opt.sgm && multi, "--aggregation sgm" + with_multi},
        {opt.bp && (opt.rgb || opt.cscale || multi),
         "--aggregation bp cannot be combined with --guidance rgb, --cross-scale, --ngpu or --pipeline"},
        {opt.bp && labels > SMX_BP_MAX_D, "--aggregation bp takes at most " + std::to_string(SMX_BP_MAX_D) + " labels"},
        {opt.rgb && (opt.sgm || multi), "--guidance rgb cannot be combined with --aggregation sgm, --ngpu or --pipeline"},
        {opt.so && (opt.rgb || multi), std::string("--aggregation ") + (opt.cross ? "cross-scanline" : "scanline") +
                                           " cannot be combined with --guidance rgb, --ngpu or --pipeline"},
        {opt.so && labels > SMX_SGM_MAX_D, std::string("--aggregation ") + (opt.cross ? "cross-scanline" : "scanline") +
                                               " takes at most " + std::to_string(SMX_SGM_MAX_D) + " labels"},
        {opt.cross && (opt.rgb || multi), "--aggregation cross cannot be combined with --guidance rgb, --ngpu or --pipeline"},
        {opt.census && multi, "--cost census" + with_multi},
        {opt.adcensus && multi, "--cost adcensus" + with_multi},
        {opt.mi && multi, "--cost mi" + with_multi},
        {opt.sgm && labels > SMX_SGM_MAX_D, "--aggregation sgm takes at most " + std::to_string(SMX_SGM_MAX_D) + " labels"},
        {opt.speckle && multi, "--speckle" + with_multi},
        {uniq && multi, "--uniqueness" + with_multi},
        {opt.vote && multi, "--vote" + with_multi},
        {opt.vote && labels > 512, "--vote takes at most 512 labels"},
        {opt.cscale && (opt.sgm || opt.cross || opt.so),
         "--cross-scale belongs to the guided filter: it cannot be combined with --aggregation sgm, cross, scanline or cross-scanline"},
        {opt.cscale && multi, "--cross-scale" + with_multi},
        {opt.perm && multi, "--permeability" + with_multi},
        {opt.pm && (opt.census || opt.adcensus), "--aggregation patchmatch scores planes with the reference's cost: it cannot be "
                                                 "combined with --cost census or adcensus"},
        {opt.pm && (opt.rgb || opt.cscale || opt.adjust || uniq),
         "--aggregation patchmatch keeps no cost volume: it cannot be combined with --guidance rgb, --cross-scale, --adjust or "
         "--uniqueness"},
        {opt.pm && opt.subpixel, "--aggregation patchmatch cannot be combined with --subpixel: its planes are sub-pixel already"},
        {opt.pm && multi, "--aggregation patchmatch" + with_multi},
        {opt.adjust && multi, "--adjust" + with_multi},
        {opt.adjust && labels > 512, "--adjust takes at most 512 labels"},
        {opt.ngpu < 0 || opt.ngpu > smx_device_count(),
         "--ngpu " + std::to_string(opt.ngpu) + ": this node shows " + std::to_string(smx_device_count()) + " HIP device(s)"}};
    for (const Rule& r : refusals)
        if (r.refused) {
            std::fprintf(stderr, "%s\n", r.message.c_str());
            return 2;
        }
    Sharded sharded;
    if (opt.ngpu >= 1 && !sharded.load()) {
        std::fprintf(stderr, "--ngpu: cannot load the sharded context of libsmx_rccl.so (%s)\n", dlerror());
        return 1;
    }
    const bool fused = opt.fused || sharded.create || opt.subpixel || opt.census || opt.adcensus || opt.mi || opt.sgm || opt.bp || uniq || opt.rgb ||
                       opt.cross || opt.so || opt.adjust || opt.cscale || opt.pm || opt.perm;
    if (opt.pairs < 1 || (opt.pairs > 1 && !fused)) {
        std::fprintf(stderr, "--pairs needs a count >= 1 and --fused or --ngpu\n");
        return 2;
    }

    // ---- load
    const std::clock_t t_begin = std::clock();
    Pair& in = job.in;
    if (!load_pair(left, right, in)) {
        std::fprintf(stderr, "cannot load an RGB pair of equal size from %s / %s\n", left.c_str(),
                     right.c_str());
        return 1;
    }
    const int w = job.w = in.w, h = job.h = in.h, n = job.n = w * h;
    if ((opt.rgb || opt.ad_rgb || opt.cross || opt.so) && (in.channels[0] != in.channels[1] || in.channels[0] > 4)) {
        std::fprintf(stderr, "%s needs two images of 3 or of 4 channels, not %d and %d\n",
                     opt.rgb ? "--guidance rgb" : opt.so ? "--aggregation scanline" : opt.cross ? "--aggregation cross" : "--ad rgb",
                     in.channels[0], in.channels[1]);
        return 1;
    }
    std::cout << "Resolution : " << w << "x" << h << std::endl;

    // ---- gray
    std::cout << "RGB to grayscale ..." << std::endl;
    for (int v = 0; v < 2; ++v) job.gray[v] = rgb_to_grayscale(in.rgb[v], n, in.channels[v], host_compare);

    // ---- the pair: the reference's stage-by-stage flow, or the device-resident one
    Maps maps(n);
    smx_stage_ms stage_ms = {};
    bool have_stage_ms = false;
    if (fused) have_stage_ms = run_device_resident(job, sharded, maps, stage_ms);
    else run_stage_by_stage(job, maps);

    // ---- not in the reference: the weighted-median refinement of the filled left map (guide: the left gray image)
    if (!opt.wmf.empty()) {
        std::cout << "weighted median ..." << std::endl;
        maps.refined.resize(n);
        // whose test says what the fill replaced
        std::vector<float>& kept = opt.speckle ? maps.despeckled : uniq ? maps.unique : maps.occlusion;
        weighted_median(job.gray[0], maps.filled.data(), opt.wmf == "occluded" ? kept.data() : nullptr, maps.refined.data(), w,
                        h, d_lo, job.size_d, host_compare);
    }
    const double duration = (std::clock() - t_begin) / (double)CLOCKS_PER_SEC;

    // ---- write
    std::cout << "writing images ..." << std::endl;
    const int write_failures = write_outputs(job, maps, outdir);

    // ---- report
    std::cout << "duration: " << duration << std::endl;
    // (the reference prints one wall-clock duration, main.cu:184; the device time of the last pair by stage goes beside it)
    if (have_stage_ms)
        std::printf("device ms of the last pair: upload %.3f, guidance %.3f, aggregation %.3f, wta %.3f, finish %.3f, "
                    "download %.3f, total %.3f\n", stage_ms.upload, stage_ms.guidance, stage_ms.aggregation, stage_ms.wta,
                    stage_ms.finish, stage_ms.download, stage_ms.total);
    std::cout << "Free the memory ..." << std::endl;
    for (int v = 0; v < 2; ++v) { std::free(job.gray[v]); std::free(in.rgb[v]); }
    if (write_failures) {
        std::fprintf(stderr, "%d output file(s) could not be written (does %s exist?)\n", write_failures, outdir.c_str());
        return 1;
    }
    return 0;
}
