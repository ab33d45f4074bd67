// main.cpp -- drop-in for the reference's entry point (stereo_matching_cuda/main.cu:37-214).
// Same stage order, same progress lines on stdout, same 12 output images, and every stage goes
// through the reference-named host functions of this directory (which forward to the HIP kernels
// behind include/smx.h).  The code itself is organised differently: buffers are std::vectors, the
// outputs are table driven, and the image normaliser (helpers.cuh) is a two-pass restatement of write_mat.
//
//   smx_main                         reference behaviour: ./data/tsukuba0.png, ./data/tsukuba1.png,
//                                    D_MIN..D_MAX from the macros, outputs into ./data/
//   smx_main L.png R.png [dmin dmax [outdir]] [options]
// options (not in the reference):
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
//                     Not with --wmf, --ngpu or --pipeline
//   --cost census     the census / Hamming matching cost instead of the reference's (smx_ctx_set_cost; implies --fused): the
//                     same twelve images, the two cost images from the census volumes.  --census-window WxH gives the
//                     window in pixels (odd, 3x3 .. 9x7; default 9x7), --census-th N the truncation (>= 1; default 62).
//                     Composes with --wmf, --subpixel, --pfm and --png16; not with --ngpu or --pipeline
//   --cost adcensus   AD-Census, census plus absolute differences, each through 1 - exp(-c / lambda) (smx_ctx_set_adcensus;
//                     implies --fused): the cost for pairs whose repeating patterns the census cost alone ties on.  The same
//                     twelve images, the two cost images from the AD-Census volumes.  --census-window / --census-th apply to its
//                     census part; --adcensus-lambda C,A gives the two lambda (0 < lambda <= 1e6; default 30,10),
//                     --adcensus-scale S the scale (2^-20 .. 2^20; default 127.5), --ad gray|rgb the images of the absolute
//                     difference: the gray ones (default) or R, G, B of the PNGs (smx_ctx_stereo_pair_rgb).  With
//                     --host-compare the CPU twin (adcensus_costOnCPU) redoes the cost images.  Composes with --aggregation
//                     sgm, --guidance rgb, --subpixel, --uniqueness, --speckle, --wmf, --pfm and --png16; not with --ngpu or
//                     --pipeline
//   --speckle SIZE[,DIFF]  speckle removal between the LR check and the fill (smx_speckle_filter; not in the reference), on
//                     every single-GPU path: connected components of at most SIZE pixels whose 4-neighbours differ by at
//                     most DIFF (default 1) are invalidated like LR failures.  Writes occlu_mapl_despeckled.png beside
//                     the 12 images; occlu_mapl_filled.png (and --wmf occluded, --subpixel, --pfm, --png16 behind it) then
//                     come from the despeckled map.  Composes with --wmf, --subpixel, --cost census; not with --ngpu or
//                     --pipeline
//   --aggregation sgm semi-global matching instead of the guided filter (smx_ctx_set_aggregation; implies --fused, and the
//                     census cost, --census-window / --census-th included, unless --cost reference is given): the same
//                     twelve images, the two mean images empty.
//                     --sgm-p P1,P2 gives the penalties (0 <= P1 <= P2 <= 4095; default 10,120), --sgm-paths 4|8 the number
//                     of directions (default 8).  With --host-compare the CPU twin (sgm_aggregateOnCPU) redoes both
//                     views from the cost volumes and check_errors compares.  At most 256 labels.  Composes with --wmf,
//                     --subpixel, --speckle, --pfm and --png16; not with --ngpu or --pipeline
//   --uniqueness PCT  the uniqueness (peak-ratio) test between the LR check and speckle removal (smx_ctx_set_uniqueness; not
//                     in the reference; implies --fused): 0 <= PCT < 100 is OpenCV's uniquenessRatio, i.e. the ratio
//                     PCT / (100 - PCT); 0 is off.  A left pixel whose winner has a non-neighbouring disparity that costs less
//                     than (1 + ratio) times as much is invalidated like an LR failure.  Writes occlu_mapl_unique.png beside
//                     the 12 images; the later stages start from that map.  With --host-compare the CPU twin
//                     (uniqueness_onCPU: brute force over the left aggregated volume) redoes it.  Composes with --cost
//                     census, --aggregation sgm, --speckle, --subpixel, --wmf, --pfm and --png16; not with --ngpu or
//                     --pipeline
//   --guidance rgb    the guided filter with the colour images as its guide instead of the gray ones (smx_ctx_set_guidance,
//                     smx_ctx_stereo_pair_rgb; not in the reference; implies --fused): an edge between two colours of equal
//                     luminance stays an edge.  The same twelve images, the two mean images empty.  With --host-compare the
//                     CPU twin (colour_guided_filterOnCPU) redoes both views from the cost volumes and check_errors
//                     compares.  Composes with --cost census, --subpixel, --uniqueness, --speckle, --wmf, --pfm and --png16;
//                     not with --aggregation sgm, --ngpu or --pipeline
//   --aggregation cross  cross-based aggregation instead of the guided filter (smx_ctx_set_cross, smx_ctx_stereo_pair_rgb; not in
//                     the reference; implies --fused): colour-adaptive support regions whose guide is the colour pair.  The same
//                     twelve images, the two mean images empty.  --cross-arms L1,L2 gives the arm lengths (1 <= L1 <= 63,
//                     0 <= L2 <= L1; default 34,17), --cross-tau T1,T2 the colour thresholds (1 <= T2 <= T1 <= 256; default
//                     20,6), --cross-iterations N the iterations (1 .. 4; default 4).  With --host-compare the CPU twin
//                     (cross_aggregateOnCPU) redoes both views from the cost volumes and check_errors compares.  Composes with
//                     --cost census / adcensus, --subpixel, --uniqueness, --speckle, --wmf, --pfm and --png16; not with
//                     --guidance rgb, --ngpu or --pipeline
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
#include <vector>

#include "adcensus.cuh"
#include "census.cuh"
#include "colourGuidedFilter.cuh"
#include "costVolume.cuh"
#include "filter.cuh"
#include "guidedFilter.cuh"
#include "helpers.cuh"
#include "occlusion.cuh"
#include "png_io.h"
#include "rgb_to_grayscale.cuh"
#include "crossAggregation.cuh"
#include "sgm.cuh"
#include "speckle.cuh"
#include "uniqueness.cuh"
#include "winner_take_all.cuh"
#include "wmf.cuh"

namespace {

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

struct Options {
    std::vector<std::string> positional;
    bool fused = false, host_compare = false, fast = false;
    std::string pfm, png16;
    std::string wmf;         // "" = no refinement, else "occluded" or "all"
    int subpixel = 0;        // 0 = off, else SMX_SUBPIX_PARABOLA / SMX_SUBPIX_EQUIANGULAR
    bool census = false;     // --cost census
    smx_census_params census_params;
    bool cost_given = false; // --cost seen
    bool adcensus = false;   // --cost adcensus
    bool ad_rgb = false;     // --ad rgb: the absolute differences on R, G, B of the colour images
    smx_adcensus_params adc_params;     // (its census part is filled from census_params after the parse)
    bool sgm = false;        // --aggregation sgm
    smx_sgm_params sgm_params;
    bool cross = false;      // --aggregation cross
    smx_cross_params cross_params;
    bool speckle = false;    // --speckle
    smx_speckle_params speckle_params;
    bool rgb = false;        // --guidance rgb
    float uniqueness = 0.0f; // --uniqueness PCT as the ratio PCT / (100 - PCT); 0 = off
    int ngpu = 0;            // 0 = not given: the single-GPU paths
    int pairs = 1;
    bool pipeline = false;
    bool overlap = false;
    bool ok = true;
};

Options parse(int argc, char** argv) {
    Options o;
    smx_default_census_params(&o.census_params);
    smx_default_speckle_params(&o.speckle_params);
    smx_default_sgm_params(&o.sgm_params);
    smx_default_cross_params(&o.cross_params);
    bool sgm_option = false;        // --sgm-p / --sgm-paths seen
    bool cross_option = false;      // --cross-arms / --cross-tau / --cross-iterations seen
    bool census_option = false;     // --census-window / --census-th seen
    bool adcensus_option = false;   // --adcensus-lambda / --adcensus-scale / --ad seen
    smx_default_adcensus_params(&o.adc_params);
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto value = [&](std::string& dst) {
            if (i + 1 < argc) dst = argv[++i];
            else { std::fprintf(stderr, "%s needs a value\n", a.c_str()); o.ok = false; }
        };
        if (a == "--fused") o.fused = true;
        else if (a == "--host-compare") o.host_compare = true;
        else if (a == "--fast") o.fast = true;
        else if (a == "--pfm") value(o.pfm);
        else if (a == "--png16") value(o.png16);
        else if (a == "--wmf") {
            value(o.wmf);
            if (o.ok && o.wmf != "occluded" && o.wmf != "all") {
                std::fprintf(stderr, "--wmf needs `occluded` or `all`, not `%s`\n", o.wmf.c_str());
                o.ok = false;
            }
        }
        else if (a == "--subpixel") {
            std::string v;
            value(v);
            o.subpixel = v == "parabola" ? SMX_SUBPIX_PARABOLA : v == "equiangular" ? SMX_SUBPIX_EQUIANGULAR : 0;
            if (o.ok && !o.subpixel) {
                std::fprintf(stderr, "--subpixel needs `parabola` or `equiangular`, not `%s`\n", v.c_str());
                o.ok = false;
            }
        }
        else if (a == "--cost") {
            std::string v;
            value(v);
            o.cost_given = true;
            o.census = v == "census";
            o.adcensus = v == "adcensus";
            if (o.ok && !o.census && !o.adcensus && v != "reference") {
                std::fprintf(stderr, "--cost needs `reference`, `census` or `adcensus`, not `%s`\n", v.c_str());
                o.ok = false;
            }
        }
        else if (a == "--adcensus-lambda") {
            std::string v;
            value(v);
            double lc = 0, la = 0;
            char comma = 0, rest = 0;
            adcensus_option = true;
            if (o.ok && (std::sscanf(v.c_str(), "%lf%c%lf%c", &lc, &comma, &la, &rest) != 3 || comma != ',' || !(lc > 0) ||
                         !(lc <= 1e6) || !(la > 0) || !(la <= 1e6))) {
                std::fprintf(stderr, "--adcensus-lambda needs C,A with 0 < C, A <= 1e6, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.adc_params.lambda_census = lc; o.adc_params.lambda_ad = la;
        }
        else if (a == "--adcensus-scale") {
            std::string v;
            value(v);
            char* end = nullptr;
            const double sc = std::strtod(v.c_str(), &end);
            adcensus_option = true;
            if (o.ok && (v.empty() || *end || !(sc >= 1.0 / 1048576.0) || !(sc <= 1048576.0))) {
                std::fprintf(stderr, "--adcensus-scale needs a scale S with 2^-20 <= S <= 2^20, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.adc_params.scale = sc;
        }
        else if (a == "--ad") {
            std::string v;
            value(v);
            adcensus_option = true;
            o.ad_rgb = v == "rgb";
            if (o.ok && !o.ad_rgb && v != "gray") {
                std::fprintf(stderr, "--ad needs `gray` or `rgb`, not `%s`\n", v.c_str());
                o.ok = false;
            }
        }
        else if (a == "--census-window") {
            std::string v;
            value(v);
            int ww = 0, wh = 0;
            char x = 0, rest = 0;
            census_option = true;
            if (o.ok && (std::sscanf(v.c_str(), "%d%c%d%c", &ww, &x, &wh, &rest) != 3 || x != 'x' || ww < 3 || ww > 9 ||
                         wh < 3 || wh > 7 || ww % 2 == 0 || wh % 2 == 0)) {
                std::fprintf(stderr, "--census-window needs WxH with odd W in 3 .. 9 and odd H in 3 .. 7, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.census_params.rx = ww / 2; o.census_params.ry = wh / 2;
        }
        else if (a == "--census-th") {
            std::string v;
            value(v);
            char* end = nullptr;
            const long th = std::strtol(v.c_str(), &end, 10);
            census_option = true;
            if (o.ok && (v.empty() || *end || th < 1 || th > 1000000)) {
                std::fprintf(stderr, "--census-th needs an integer >= 1, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.census_params.th = (int)th;
        }
        else if (a == "--aggregation") {
            std::string v;
            value(v);
            o.sgm = v == "sgm";
            o.cross = v == "cross";
            if (o.ok && !o.sgm && !o.cross && v != "guided") {
                std::fprintf(stderr, "--aggregation needs `guided`, `sgm` or `cross`, not `%s`\n", v.c_str());
                o.ok = false;
            }
        }
        else if (a == "--cross-arms") {
            std::string v;
            value(v);
            int l1 = -1, l2 = -1;
            char comma = 0, rest = 0;
            cross_option = true;
            if (o.ok && (std::sscanf(v.c_str(), "%d%c%d%c", &l1, &comma, &l2, &rest) != 3 || comma != ',' || l1 < 1 || l1 > 63 ||
                         l2 < 0 || l2 > l1)) {
                std::fprintf(stderr, "--cross-arms needs L1,L2 with 1 <= L1 <= 63 and 0 <= L2 <= L1, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.cross_params.l1 = l1; o.cross_params.l2 = l2;
        }
        else if (a == "--cross-tau") {
            std::string v;
            value(v);
            int t1 = -1, t2 = -1;
            char comma = 0, rest = 0;
            cross_option = true;
            if (o.ok && (std::sscanf(v.c_str(), "%d%c%d%c", &t1, &comma, &t2, &rest) != 3 || comma != ',' || t2 < 1 || t2 > t1 ||
                         t1 > 256)) {
                std::fprintf(stderr, "--cross-tau needs T1,T2 with 1 <= T2 <= T1 <= 256, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.cross_params.tau1 = t1; o.cross_params.tau2 = t2;
        }
        else if (a == "--cross-iterations") {
            std::string v;
            value(v);
            cross_option = true;
            if (o.ok && v != "1" && v != "2" && v != "3" && v != "4") {
                std::fprintf(stderr, "--cross-iterations needs 1, 2, 3 or 4, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.cross_params.iterations = o.ok ? v[0] - '0' : 0;
        }
        else if (a == "--sgm-p") {
            std::string v;
            value(v);
            int p1 = -1, p2 = -1;
            char comma = 0, rest = 0;
            sgm_option = true;
            if (o.ok && (std::sscanf(v.c_str(), "%d%c%d%c", &p1, &comma, &p2, &rest) != 3 || comma != ',' || p1 < 0 || p1 > p2 ||
                         p2 > 4095)) {
                std::fprintf(stderr, "--sgm-p needs P1,P2 with 0 <= P1 <= P2 <= 4095, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.sgm_params.p1 = p1; o.sgm_params.p2 = p2;
        }
        else if (a == "--sgm-paths") {
            std::string v;
            value(v);
            sgm_option = true;
            if (o.ok && v != "4" && v != "8") {
                std::fprintf(stderr, "--sgm-paths needs 4 or 8, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.sgm_params.paths = v == "4" ? 4 : 8;
        }
        else if (a == "--speckle") {
            std::string v;
            value(v);
            int size = -1;
            float diff = 1.0f;
            char comma = 0, rest = 0;
            const int got = std::sscanf(v.c_str(), "%d%c%f%c", &size, &comma, &diff, &rest);
            o.speckle = true;
            if (o.ok && (!(got == 1 || (got == 3 && comma == ',')) || size < 0 || !(diff >= 0.0f) || !(diff <= 3.4e38f))) {
                std::fprintf(stderr, "--speckle needs SIZE[,DIFF] with SIZE >= 0 and a finite DIFF >= 0, not `%s`\n", v.c_str());
                o.ok = false;
            }
            o.speckle_params.max_size = size; o.speckle_params.max_diff = diff;
        }
        else if (a == "--uniqueness") {
            std::string v;
            value(v);
            char* end = nullptr;
            const float pct = std::strtof(v.c_str(), &end);
            if (o.ok && (v.empty() || *end || !(pct >= 0.0f) || !(pct < 100.0f))) {
                std::fprintf(stderr, "--uniqueness needs a percentage PCT with 0 <= PCT < 100, not `%s`\n", v.c_str());
                o.ok = false;
            }
            if (o.ok) o.uniqueness = pct / (100.0f - pct);
        }
        else if (a == "--guidance") {
            std::string v;
            value(v);
            o.rgb = v == "rgb";
            if (o.ok && !o.rgb && v != "gray") {
                std::fprintf(stderr, "--guidance needs `gray` or `rgb`, not `%s`\n", v.c_str());
                o.ok = false;
            }
        }
        else if (a == "--ngpu") { std::string v; value(v); o.ngpu = std::atoi(v.c_str()); }
        else if (a == "--pipeline") o.pipeline = true;
        else if (a == "--pairs") { std::string v; value(v); o.pairs = std::atoi(v.c_str()); }
        else if (a == "--overlap") o.overlap = true;
        else if (a.rfind("--", 0) == 0) { std::fprintf(stderr, "unknown option %s\n", a.c_str()); o.ok = false; }
        else o.positional.push_back(a);
    }
    if (o.sgm && !o.cost_given) o.census = true;     // census + SGM is the standard pairing
    if (o.ok && census_option && !o.census && !o.adcensus) {     // (after the line above: the census options go with the implied cost too)
        std::fprintf(stderr, "--census-window and --census-th need the census cost (--cost census, or --aggregation sgm "
                             "without --cost reference) or --cost adcensus\n");
        o.ok = false;
    }
    if (o.ok && adcensus_option && !o.adcensus) {
        std::fprintf(stderr, "--adcensus-lambda, --adcensus-scale and --ad need --cost adcensus\n");
        o.ok = false;
    }
    o.adc_params.census = o.census_params;
    o.adc_params.colour = o.ad_rgb ? 1 : 0;
    if (o.ok && sgm_option && !o.sgm) {
        std::fprintf(stderr, "--sgm-p and --sgm-paths need --aggregation sgm\n");
        o.ok = false;
    }
    if (o.ok && cross_option && !o.cross) {
        std::fprintf(stderr, "--cross-arms, --cross-tau and --cross-iterations need --aggregation cross\n");
        o.ok = false;
    }
    return o;
}

}  // namespace

int main(int argc, char** argv) {
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
    const int d_lo = smx_config().d_min, d_hi = smx_config().d_max;
    if (d_hi < d_lo || (long long)d_hi - d_lo + 1 > 4096) {
        std::fprintf(stderr, "bad disparity range [%d, %d]: need dmin <= dmax and at most 4096 labels\n", d_lo, d_hi);
        return 2;
    }
    if (opt.subpixel && (!opt.wmf.empty() || opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--subpixel cannot be combined with --wmf (the median works on integer labels), --ngpu or "
                             "--pipeline\n");
        return 2;
    }
    // (before the census refusal: SGM implies the census cost, and the message names the option that was given)
    if (opt.sgm && (opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--aggregation sgm cannot be combined with --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.rgb && (opt.sgm || opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--guidance rgb cannot be combined with --aggregation sgm, --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.cross && (opt.rgb || opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--aggregation cross cannot be combined with --guidance rgb, --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.census && (opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--cost census cannot be combined with --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.adcensus && (opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--cost adcensus cannot be combined with --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.sgm && (long long)d_hi - d_lo + 1 > SMX_SGM_MAX_D) {
        std::fprintf(stderr, "--aggregation sgm takes at most %d labels\n", SMX_SGM_MAX_D);
        return 2;
    }
    if (opt.speckle && (opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--speckle cannot be combined with --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.uniqueness > 0.0f && (opt.ngpu != 0 || opt.pipeline)) {
        std::fprintf(stderr, "--uniqueness cannot be combined with --ngpu or --pipeline\n");
        return 2;
    }
    if (opt.ngpu < 0 || opt.ngpu > smx_device_count()) {
        std::fprintf(stderr, "--ngpu %d: this node shows %d HIP device(s)\n", opt.ngpu, smx_device_count());
        return 2;
    }
    // the multi-GPU driver (RCCL) is loaded only when asked for, so the plain binary does not need librccl
    typedef int (*sh_create_fn)(const smx_params*, int, int, int, int, int, void**);
    typedef int (*sh_run_fn)(void*, const uint8_t*, const uint8_t*, int, int, const smx_pair_out*);
    typedef int (*sh_destroy_fn)(void*);
    sh_create_fn sh_create = nullptr;
    sh_run_fn sh_run = nullptr;
    sh_destroy_fn sh_destroy = nullptr;
    if (opt.ngpu >= 1) {
        void* so = dlopen("libsmx_rccl.so", RTLD_NOW | RTLD_LOCAL);
        sh_create = so ? (sh_create_fn)dlsym(so, "smx_sharded_create") : nullptr;
        sh_run = so ? (sh_run_fn)dlsym(so, "smx_sharded_run") : nullptr;
        sh_destroy = so ? (sh_destroy_fn)dlsym(so, "smx_sharded_destroy") : nullptr;
        if (!sh_create || !sh_run || !sh_destroy) {
            std::fprintf(stderr, "--ngpu: cannot load the sharded context of libsmx_rccl.so (%s)\n", dlerror());
            return 1;
        }
    }
    const bool uniq = opt.uniqueness > 0.0f;
    const bool fused = opt.fused || sh_create || opt.subpixel || opt.census || opt.adcensus || opt.sgm || uniq || opt.rgb || opt.cross;
    if (opt.pairs < 1 || (opt.pairs > 1 && !fused)) {
        std::fprintf(stderr, "--pairs needs a count >= 1 and --fused or --ngpu\n");
        return 2;
    }

    const std::clock_t t_begin = std::clock();
    bool have_stage_ms = false;
    smx_stage_ms stage_ms = {};
    Pair in;
    if (!load_pair(left, right, in)) {
        std::fprintf(stderr, "cannot load an RGB pair of equal size from %s / %s\n", left.c_str(),
                     right.c_str());
        return 1;
    }
    const int w = in.w, h = in.h, n = w * h;
    if ((opt.rgb || opt.ad_rgb || opt.cross) && (in.channels[0] != in.channels[1] || in.channels[0] > 4)) {
        std::fprintf(stderr, "%s needs two images of 3 or of 4 channels, not %d and %d\n",
                     opt.rgb ? "--guidance rgb" : opt.cross ? "--aggregation cross" : "--ad rgb",
                     in.channels[0], in.channels[1]);
        return 1;
    }
    std::cout << "Resolution : " << w << "x" << h << std::endl;

    std::cout << "RGB to grayscale ..." << std::endl;
    unsigned char* gray[2] = {rgb_to_grayscale(in.rgb[0], n, in.channels[0], host_compare),
                              rgb_to_grayscale(in.rgb[1], n, in.channels[1], host_compare)};

    // left volume: labels d_lo .. d_hi; right volume: labels -d_hi .. -d_lo   (main.cu:79-82)
    const int size_d = d_hi - d_lo + 1;
    const int dmin[2] = {d_lo, -d_hi};
    // --cost adcensus: the images of its absolute differences, and their bytes per pixel
    unsigned char* const ad_img[2] = {opt.ad_rgb ? in.rgb[0] : gray[0], opt.ad_rgb ? in.rgb[1] : gray[1]};
    const int ad_ch = opt.ad_rgb ? in.channels[0] : 1;
    // WTA presets of main.cu:112-118: memset(best, 9999999.0f) stores byte 0x7F everywhere
    std::vector<float> best[2], dmap[2], cost[2];
    std::vector<unsigned char> mean[2], unused_u8[2];
    for (int v = 0; v < 2; ++v) {
        best[v].resize(n);
        std::memset(best[v].data(), 0x7F, sizeof(float) * n);
        dmap[v].assign(n, 0.0f);
        mean[v].assign(n, 0);
        unused_u8[v].assign(n, 0);
    }
    std::vector<float> occlusion, filled;
    std::vector<float> sub_filled;     // --subpixel: the sub-pixel filled left map
    std::vector<float> despeckled;     // --speckle: the LR-checked left map without its small components
    std::vector<float> unique;         // --uniqueness: the LR-checked left map without its ambiguous winners
    if (!fused) {
        // the reference's data flow: every stage is a host -> device -> host round trip
        for (int v = 0; v < 2; ++v) cost[v].resize((size_t)n * size_d);
        std::cout << "Cost Volume ..." << std::endl;
        compute_cost(gray[0], gray[1], cost[0].data(), w, w, h, h, dmin[0], host_compare);
        compute_cost(gray[1], gray[0], cost[1].data(), w, w, h, h, dmin[1], host_compare);
        std::cout << "guided filter ..." << std::endl;
        for (int v = 0; v < 2; ++v)
            compute_guided_filter(gray[v], cost[v].data(), best[v].data(), dmap[v].data(), mean[v].data(), w, h,
                                  size_d, dmin[v], host_compare);
        std::cout << "guided filter ok" << std::endl;
        // left-right check on a copy of the left map, then scan-line filling on a copy of that
        occlusion = dmap[0];
        detect_occlusion(occlusion.data(), dmap[1].data(), dmin[0] - 100, unused_u8[0].data(),
                         unused_u8[1].data(), w, h);                                   // main.cu:149-150
        if (opt.speckle) {
            despeckled.resize(n);
            speckle_filter(occlusion.data(), despeckled.data(), w, h, (float)d_lo, (float)(d_lo - 100), opt.speckle_params,
                           host_compare);
        }
        filled = opt.speckle ? despeckled : occlusion;
        fill_occlusion(filled.data(), w, h, (float)d_lo);                              // main.cu:154-155
    } else {
        // device-resident: one call, the cost slices never leave the CU (only slice 0 of each volume
        // is materialised, for the two cost images the reference writes)
        std::cout << "Cost Volume ..." << std::endl;
        for (int v = 0; v < 2; ++v) cost[v].resize((size_t)n);
        if (opt.adcensus) {
            for (int v = 0; v < 2; ++v)
                compute_adcensus_cost(ad_img[v], ad_img[1 - v], ad_ch, cost[v].data(), w, h, 1, dmin[v], opt.adc_params, host_compare);
        } else if (opt.census) {
            compute_census_cost(gray[0], gray[1], cost[0].data(), w, h, 1, dmin[0], opt.census_params);
            compute_census_cost(gray[1], gray[0], cost[1].data(), w, h, 1, dmin[1], opt.census_params);
        } else {
            CHECK(smx_compute_cost(&smx_config().params, gray[0], gray[1], cost[0].data(), w, w, h, h, 1, dmin[0]));
            CHECK(smx_compute_cost(&smx_config().params, gray[1], gray[0], cost[1].data(), w, w, h, h, 1, dmin[1]));
        }
        std::cout << "guided filter ..." << std::endl;
        occlusion.resize(n);
        filled.resize(n);
        smx_pair_out out;
        std::memset(&out, 0, sizeof(out));
        out.best_l = best[0].data(); out.best_r = best[1].data();
        out.dmap_l = dmap[0].data(); out.dmap_r = dmap[1].data();
        // (SGM, the colour guide and cross-based aggregation have no mean images)
        if (!opt.sgm && !opt.rgb && !opt.cross) { out.mean_l = mean[0].data(); out.mean_r = mean[1].data(); }
        out.occlusion = occlusion.data(); out.filled = filled.data();
        std::vector<float> agg_l;          // the left aggregated volume: what the uniqueness twin reads
        if (uniq && host_compare) {
            agg_l.resize((size_t)n * size_d);
            out.agg_l = agg_l.data();
        }
        // one persistent context for all pairs: nothing is allocated, created or destroyed per pair
        void* sctx = nullptr;
        smx_ctx* ctx = nullptr;
        if (sh_create) CHECK(sh_create(&smx_config().params, w, h, size_d, opt.ngpu, opt.overlap ? 1 : 0, &sctx));
        else CHECK(smx_create(&smx_config().params, w, h, size_d, &ctx));
        if (opt.subpixel) CHECK(smx_ctx_set_subpixel(ctx, opt.subpixel));
        if (opt.census) CHECK(smx_ctx_set_cost(ctx, SMX_COST_CENSUS, &opt.census_params));
        if (opt.adcensus) CHECK(smx_ctx_set_adcensus(ctx, &opt.adc_params));
        if (opt.speckle) CHECK(smx_ctx_set_speckle(ctx, &opt.speckle_params));
        if (uniq) CHECK(smx_ctx_set_uniqueness(ctx, opt.uniqueness));
        if (opt.sgm) CHECK(smx_ctx_set_aggregation(ctx, SMX_AGG_SGM, &opt.sgm_params));
        if (opt.rgb) CHECK(smx_ctx_set_guidance(ctx, SMX_GUIDE_RGB));
        if (opt.cross) CHECK(smx_ctx_set_cross(ctx, &opt.cross_params));      // (its guide: the colour pair)
        if (!sh_create) CHECK(smx_set_timing(1));     // per-stage device times of the last pair (smx_stage_times)
        auto run_pair = [&]() {
            return sh_create ? sh_run(sctx, gray[0], gray[1], dmin[0], dmin[1], &out)
                   : opt.rgb || opt.ad_rgb || opt.cross ? smx_ctx_stereo_pair_rgb(ctx, in.rgb[0], in.rgb[1], in.channels[0], dmin[0], dmin[1], &out)
                             : smx_ctx_stereo_pair(ctx, gray[0], gray[1], dmin[0], dmin[1], &out);
        };
        CHECK(run_pair());
        if (opt.pairs > 1 && opt.pipeline && !sh_create) {
            // two pairs in flight; every result is copied out of the staging into the same output buffers
            const auto t0 = std::chrono::steady_clock::now();
            for (int k = 1; k < opt.pairs; ++k) {
                CHECK(smx_ctx_stereo_pair_async(ctx, gray[0], gray[1], dmin[0], dmin[1]));
                if (k >= 2) CHECK(smx_ctx_wait(ctx, nullptr, &out));
            }
            CHECK(smx_ctx_wait(ctx, nullptr, &out));
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::printf("pairs %d on one context: %.3f ms per pair, uploads and downloads included (pipelined entry)\n",
                        opt.pairs - 1, ms / (opt.pairs - 1));
        } else if (opt.pairs > 1) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int k = 1; k < opt.pairs; ++k) CHECK(run_pair());
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::printf("pairs %d on one context: %.3f ms per pair, uploads and downloads included\n", opt.pairs - 1,
                        ms / (opt.pairs - 1));
        }
        if (!sh_create) {
            smx_stage_ms t;
            if (smx_stage_times(&t) == SMX_OK) {
                have_stage_ms = true;
                stage_ms = t;
            }
            CHECK(smx_set_timing(0));
        }
        if (opt.subpixel) {
            sub_filled.resize(n);
            CHECK(smx_ctx_subpixel_maps(ctx, nullptr, nullptr, sub_filled.data()));
        }
        if (opt.speckle) {
            despeckled.resize(n);
            CHECK(smx_ctx_speckle_map(ctx, despeckled.data()));
        }
        if (uniq) {
            unique.resize(n);
            CHECK(smx_ctx_uniqueness_map(ctx, unique.data(), nullptr));
        }
        if (sh_create) CHECK(sh_destroy(sctx));
        else CHECK(smx_destroy(ctx));
        std::cout << "guided filter ok" << std::endl;
        if (host_compare && opt.sgm) {
            // the twin redoes both views from whole cost volumes built by the stage wrappers
            bool ok = true;
            for (int v = 0; v < 2; ++v) {
                std::vector<float> vol((size_t)n * size_d), tb(n), td(n);
                if (opt.adcensus)
                    compute_adcensus_cost(ad_img[v], ad_img[1 - v], ad_ch, vol.data(), w, h, size_d, dmin[v], opt.adc_params, false);
                else if (opt.census) compute_census_cost(gray[v], gray[1 - v], vol.data(), w, h, size_d, dmin[v], opt.census_params);
                else CHECK(smx_compute_cost(&smx_config().params, gray[v], gray[1 - v], vol.data(), w, w, h, h, size_d, dmin[v]));
                sgm_aggregateOnCPU(vol.data(), nullptr, tb.data(), td.data(), w, h, size_d, dmin[v], opt.sgm_params);
                ok = check_errors(tb.data(), best[v].data(), n) && ok;
                ok = check_errors(td.data(), dmap[v].data(), n) && ok;
            }
            if (ok) std::cout << "Semi-global matching ok!" << std::endl;
        }
        if (host_compare && opt.rgb) {
            // the twin redoes both views from whole cost volumes built by the stage wrappers, from the reference's presets
            bool ok = true;
            for (int v = 0; v < 2; ++v) {
                std::vector<float> vol((size_t)n * size_d), tb(n), td(n, 0.0f);
                std::memset(tb.data(), 0x7F, sizeof(float) * n);
                if (opt.adcensus)
                    compute_adcensus_cost(ad_img[v], ad_img[1 - v], ad_ch, vol.data(), w, h, size_d, dmin[v], opt.adc_params, false);
                else if (opt.census) compute_census_cost(gray[v], gray[1 - v], vol.data(), w, h, size_d, dmin[v], opt.census_params);
                else CHECK(smx_compute_cost(&smx_config().params, gray[v], gray[1 - v], vol.data(), w, w, h, h, size_d, dmin[v]));
                colour_guided_filterOnCPU(in.rgb[v], in.channels[v], vol.data(), tb.data(), td.data(), nullptr, w, h, size_d, dmin[v],
                                          smx_config().params.radius, smx_config().params.eps);
                ok = check_errors(tb.data(), best[v].data(), n) && ok;
                ok = check_errors(td.data(), dmap[v].data(), n) && ok;
            }
            if (ok) std::cout << "Colour guided filter ok!" << std::endl;
        }
        if (host_compare && opt.cross) {
            // the twin redoes both views from whole cost volumes built by the stage wrappers, from the reference's presets
            bool ok = true;
            for (int v = 0; v < 2; ++v) {
                std::vector<float> vol((size_t)n * size_d), tb(n), td(n, 0.0f);
                std::memset(tb.data(), 0x7F, sizeof(float) * n);
                if (opt.adcensus)
                    compute_adcensus_cost(ad_img[v], ad_img[1 - v], ad_ch, vol.data(), w, h, size_d, dmin[v], opt.adc_params, false);
                else if (opt.census) compute_census_cost(gray[v], gray[1 - v], vol.data(), w, h, size_d, dmin[v], opt.census_params);
                else CHECK(smx_compute_cost(&smx_config().params, gray[v], gray[1 - v], vol.data(), w, w, h, h, size_d, dmin[v]));
                cross_aggregateOnCPU(in.rgb[v], in.channels[v], vol.data(), tb.data(), td.data(), nullptr, w, h, size_d, dmin[v],
                                     opt.cross_params);
                ok = check_errors(tb.data(), best[v].data(), n) && ok;
                ok = check_errors(td.data(), dmap[v].data(), n) && ok;
            }
            if (ok) std::cout << "Cross-based aggregation ok!" << std::endl;
        }
        if (host_compare) {
            std::vector<float> lr(dmap[0]);
            detect_occlusionOnCPU(lr.data(), dmap[1].data(), dmin[0] - 100, w, h);
            bool ok = check_errors(lr.data(), occlusion.data(), n);
            if (uniq) {
                std::vector<float> twin(n);
                uniqueness_onCPU(agg_l.data(), lr.data(), twin.data(), nullptr, w, h, size_d, opt.uniqueness, (float)d_lo,
                                 (float)(d_lo - 100));
                const bool same = check_errors(twin.data(), unique.data(), n);
                if (same) std::cout << "Uniqueness ok!" << std::endl;
                ok = same && ok;
                lr = twin;
            }
            if (opt.speckle) {
                std::vector<float> twin(n);
                speckle_filterOnCPU(lr.data(), twin.data(), w, h, (float)d_lo, (float)(d_lo - 100), opt.speckle_params);
                ok = check_errors(twin.data(), despeckled.data(), n) && ok;
                lr = twin;
            }
            fill_occlusionOnCPU(lr.data(), w, h, (float)d_lo);
            ok = check_errors(lr.data(), filled.data(), n) && ok;
            if (ok) std::cout << "Occlusion ok!" << std::endl;
        }
    }
    // not in the reference: the weighted-median refinement of the filled left map (guide: the left gray image)
    std::vector<float> refined;
    if (!opt.wmf.empty()) {
        std::cout << "weighted median ..." << std::endl;
        refined.resize(n);
        // whose test says what the fill replaced
        float* kept = opt.speckle ? despeckled.data() : uniq ? unique.data() : occlusion.data();
        weighted_median(gray[0], filled.data(), opt.wmf == "occluded" ? kept : nullptr, refined.data(), w, h,
                        d_lo, size_d, host_compare);
    }
    const double duration = (std::clock() - t_begin) / (double)CLOCKS_PER_SEC;

    std::cout << "writing images ..." << std::endl;
    struct U8Out { const char* name; const unsigned char* data; };
    struct F32Out { const char* name; const float* data; };
    const U8Out u8_outputs[] = {{"image_left.png", gray[0]}, {"image_right.png", gray[1]},
                                {"image_mean_left.png", mean[0].data()},
                                {"image_mean_right.png", mean[1].data()}};
    // file names of the reference (its cost images are named after its default range)
    const F32Out f32_outputs[] = {{"best_costl.png", best[0].data()},       {"best_costr.png", best[1].data()},
                                  {"cost_lminus15.png", cost[0].data()},    {"cost_rminus15.png", cost[1].data()},
                                  {"occlu_mapl.png", occlusion.data()},     {"disparity_mapl.png", dmap[0].data()},
                                  {"disparity_mapr.png", dmap[1].data()},   {"occlu_mapl_filled.png", filled.data()}};
    int write_failures = 0;
    for (const U8Out& o : u8_outputs)
        if (!smx_png_write((outdir + "/" + o.name).c_str(), w, h, 1, o.data)) ++write_failures;
    for (const F32Out& o : f32_outputs) {
        const std::vector<unsigned char> img = normalise_like_reference(o.data, (size_t)n);
        if (!smx_png_write((outdir + "/" + o.name).c_str(), w, h, 1, img.data())) ++write_failures;
    }
    if (!despeckled.empty()) {
        const std::vector<unsigned char> img = normalise_like_reference(despeckled.data(), (size_t)n);
        if (!smx_png_write((outdir + "/occlu_mapl_despeckled.png").c_str(), w, h, 1, img.data())) ++write_failures;
    }
    if (!unique.empty()) {
        const std::vector<unsigned char> img = normalise_like_reference(unique.data(), (size_t)n);
        if (!smx_png_write((outdir + "/occlu_mapl_unique.png").c_str(), w, h, 1, img.data())) ++write_failures;
    }
    if (!refined.empty()) {
        const std::vector<unsigned char> img = normalise_like_reference(refined.data(), (size_t)n);
        if (!smx_png_write((outdir + "/occlu_mapl_wmf.png").c_str(), w, h, 1, img.data())) ++write_failures;
    }
    // disparity outputs in dataset conventions: positive pixel offsets of the filled left map (the refined one with --wmf,
    // the sub-pixel one with --subpixel)
    const float* final_map = !sub_filled.empty() ? sub_filled.data() : refined.empty() ? filled.data() : refined.data();
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

    std::cout << "duration: " << duration << std::endl;
    // (the reference prints one wall-clock duration, main.cu:184; the device time of the last pair by stage goes beside it)
    if (have_stage_ms)
        std::printf("device ms of the last pair: upload %.3f, guidance %.3f, aggregation %.3f, wta %.3f, finish %.3f, "
                    "download %.3f, total %.3f\n", stage_ms.upload, stage_ms.guidance, stage_ms.aggregation, stage_ms.wta,
                    stage_ms.finish, stage_ms.download, stage_ms.total);
    std::cout << "Free the memory ..." << std::endl;
    for (int v = 0; v < 2; ++v) { std::free(gray[v]); std::free(in.rgb[v]); }
    if (write_failures) {
        std::fprintf(stderr, "%d output file(s) could not be written (does %s exist?)\n", write_failures, outdir.c_str());
        return 1;
    }
    return 0;
}
