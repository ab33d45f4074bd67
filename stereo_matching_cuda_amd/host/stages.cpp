// stages.cpp -- the reference's per-stage host functions (same names, arguments and in/out
// behaviour) as thin forwards to the C-ABI of include/smx.h.  Host pointers in, host pointers out,
// synchronous, errors abort like the reference's CHECK macro.
#include "adcensus.cuh"
#include "census.cuh"
#include "costVolume.cuh"
#include "crossAggregation.cuh"
#include "discontinuityAdjustment.cuh"
#include "filter.cuh"
#include "guidedFilter.cuh"
#include "mutualInformation.cuh"
#include "occlusion.cuh"
#include "patchMatch.cuh"
#include "permeability.cuh"
#include "rgb_to_grayscale.cuh"
#include "colourGuidedFilter.cuh"
#include "scanlineOptimization.cuh"
#include "beliefPropagation.cuh"
#include "sgm.cuh"
#include "regionVoting.cuh"
#include "speckle.cuh"
#include "wmf.cuh"

#include <vector>

using namespace std;

smx_host_config& smx_config() {
    static smx_host_config c = [] {
        smx_host_config k;
        smx_default_params(&k.params);
        k.params.r_w = R_W; k.params.g_w = G_W; k.params.b_w = B_W;
        k.params.alpha = ALPHA; k.params.th_color = TH_color; k.params.th_grad = TH_grad;
        k.params.radius = RADIUS; k.params.eps = EPS; k.params.d_lr = D_LR;
        k.d_min = D_MIN; k.d_max = D_MAX;
        return k;
    }();
    return c;
}

// helpers.cu:3-25 -- exact-equality compare that reports every mismatching element
namespace {
template <class T>
bool report_mismatches(const T* expected, const T* got, int len) {
    int mismatches = 0;
    for (int k = 0; k < len; ++k) {
        if (expected[k] == got[k]) continue;
        ++mismatches;
        cout << "error at element: " << k << " ResultGPU = " << +got[k] << " and ResultCPU= " << +expected[k]
             << endl;
    }
    return mismatches == 0;
}

// What the aggregation wrappers' host_gpu_compare ends with: the twin's best costs, labels and (where asked for) aggregated
// volume against the GPU's, and the stage's line if all agree.
void compare_aggregation(const char* stage, std::vector<float>& tb, std::vector<float>& td, std::vector<float>& ta, float* best,
                         float* disp_map, float* agg, int n, int size_d) {
    bool ok = check_errors(tb.data(), best, n);
    ok = check_errors(td.data(), disp_map, n) && ok;
    if (agg) ok = check_errors(ta.data(), agg, n * size_d) && ok;
    if (ok) cout << stage << " ok!" << endl;
}
}  // namespace

bool check_errors(float* resCPU, float* resGPU, int len) { return report_mismatches(resCPU, resGPU, len); }
bool check_errors(unsigned char* resCPU, unsigned char* resGPU, int len) {
    return report_mismatches(resCPU, resGPU, len);
}

// rgb_to_grayscale.cu:25-73 (host_gpu_compare: :60-65)
unsigned char* rgb_to_grayscale(unsigned char* h_rgb, const int n, int channels, bool host_gpu_compare) {
    unsigned char* h_gray = (unsigned char*)malloc(n);
    memset(h_gray, 0, n);
    CHECK(smx_rgb_to_grayscale(&smx_config().params, h_rgb, n, channels, h_gray));
    if (host_gpu_compare) {
        std::vector<unsigned char> twin(n);
        sumArraysOnHost(h_rgb, twin.data(), n, channels);
        if (check_errors_grayscale(twin.data(), h_gray, n)) cout << "Grayscale ok!" << endl;
    }
    return h_gray;
}

// costVolume.cu:4-84 (host_gpu_compare: :56-74)
void compute_cost(unsigned char* i1, unsigned char* i2, float* cost, int w1, int w2, int h1, int h2,
                  int dmin, bool host_gpu_compare) {
    const int size_d = smx_config().d_max - smx_config().d_min + 1;   // costVolume.cu:5
    CHECK(smx_compute_cost(&smx_config().params, i1, i2, cost, w1, w2, h1, h2, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> twin((size_t)size_d * w1 * h1);
        costVolumeOnCPU(i1, i2, twin.data(), w1, w2, h1, h2, size_d, dmin);
        // (the reference-signature check_errors takes an int count: volumes beyond 2^31 cells are compared in planes)
        bool ok = true;
        for (int z = 0; z < size_d; ++z)
            ok = check_errors(twin.data() + (size_t)z * w1 * h1, cost + (size_t)z * w1 * h1, w1 * h1) && ok;
        if (ok) cout << "Cost volume ok!" << endl;
    }
}

// not in the reference: the census / Hamming cost volume (smx_main --cost census)
void compute_census_cost(unsigned char* i1, unsigned char* i2, float* cost, int w, int h, int size_d, int dmin,
                         const smx_census_params& p) {
    CHECK(smx_census_cost(&p, i1, i2, cost, w, h, size_d, dmin));
}

// not in the reference: the AD-Census cost volume (smx_main --cost adcensus)
void compute_adcensus_cost(unsigned char* i1, unsigned char* i2, int channels, float* cost, int w, int h, int size_d, int dmin,
                           const smx_adcensus_params& p, bool host_gpu_compare) {
    CHECK(smx_adcensus_cost(&p, i1, i2, channels, cost, w, h, size_d, dmin));
    if (host_gpu_compare) {
        const size_t n = (size_t)w * h;
        std::vector<float> table(SMX_ADCENSUS_TABLE_FLOATS), twin(n * size_d);
        CHECK(smx_adcensus_tables(&p, table.data()));
        std::vector<unsigned char> g1, g2;          // the gray images of the codes, made like the device makes them
        if (channels > 1) {
            g1.resize(n); g2.resize(n);
            sumArraysOnHost(i1, g1.data(), (int)n, channels);
            sumArraysOnHost(i2, g2.data(), (int)n, channels);
        }
        adcensus_costOnCPU(i1, i2, channels > 1 ? g1.data() : i1, channels > 1 ? g2.data() : i2, channels, twin.data(), w, h,
                           size_d, dmin, p, table.data());
        bool ok = true;
        for (int z = 0; z < size_d; ++z) ok = check_errors(twin.data() + (size_t)z * n, cost + (size_t)z * n, (int)n) && ok;
        if (ok) cout << "AD-Census cost ok!" << endl;
    }
}

// not in the reference: the mutual-information cost (smx_main --cost mi) -- the joint histogram of a left map, and the volume
// of one view from a table
void compute_mi_histogram(unsigned char* left, unsigned char* right, float* disp, float mark, unsigned int* hist, int w, int h,
                          bool host_gpu_compare) {
    CHECK(smx_mi_histogram(left, right, disp, mark, hist, w, h));
    if (host_gpu_compare) {
        std::vector<unsigned int> twin((size_t)SMX_MI_LEVELS * SMX_MI_LEVELS);
        mi_histogramOnCPU(left, right, disp, mark, twin.data(), w, h);
        if (std::memcmp(twin.data(), hist, twin.size() * sizeof(unsigned int)) == 0) cout << "Mutual-information histogram ok!" << endl;
        else cout << "error in the mutual-information histogram" << endl;
    }
}

void compute_mi_cost(const unsigned char* table, unsigned char* left, unsigned char* right, int view, float* cost, int w, int h,
                     int size_d, int dmin, bool host_gpu_compare) {
    CHECK(smx_mi_cost(table, view ? right : left, view ? left : right, view, cost, w, h, size_d, dmin));
    if (host_gpu_compare) {
        const size_t n = (size_t)w * h;
        std::vector<float> twin(n * size_d);
        mi_costOnCPU(table, left, right, view, twin.data(), w, h, size_d, dmin);
        bool ok = true;
        for (int z = 0; z < size_d; ++z) ok = check_errors(twin.data() + (size_t)z * n, cost + (size_t)z * n, (int)n) && ok;
        if (ok) cout << "Mutual-information cost ok!" << endl;
    }
}

// integral.cu:3-51
void integral(float* image, float* integral, int width, int height) {
    CHECK(smx_integral(image, integral, width, height));
}

// guidedFilter.cu:4-295.  host_gpu_compare: the correct CPU twin runs on copies of the in/out arrays
// and every output is compared exactly (the reference runs its twin from main.cu:136-139 and never
// looks at the result).
void compute_guided_filter(unsigned char* i, float* cost, float* filter_cost, float* disp_map,
                           unsigned char* mean, const int w, const int h, const int size_d, int dmin,
                           bool host_gpu_compare) {
    const int n = w * h;
    std::vector<float> best_twin, dmap_twin;
    if (host_gpu_compare) {
        best_twin.assign(filter_cost, filter_cost + n);
        dmap_twin.assign(disp_map, disp_map + n);
    }
    CHECK(smx_compute_guided_filter(&smx_config().params, i, cost, filter_cost, disp_map, mean,
                                    nullptr, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<unsigned char> mean_twin(n);
        guided_filter_onCpu(i, cost, best_twin.data(), dmap_twin.data(), mean_twin.data(), w, h, size_d, dmin);
        bool ok = check_errors(best_twin.data(), filter_cost, n);
        ok = check_errors(dmap_twin.data(), disp_map, n) && ok;
        if (mean) ok = check_errors(mean_twin.data(), mean, n) && ok;
        if (ok) cout << "Guided filter ok!" << endl;
    }
}

// occlusion.cu:17-85
void detect_occlusion(float* disparityLeft, float* disparityRight, const int dOcclusion,
                      unsigned char*, unsigned char*, const int w, const int h) {
    CHECK(smx_detect_occlusion(&smx_config().params, disparityLeft, disparityRight, dOcclusion, w, h));
}

// occlusion.cu:111-132
void fill_occlusion(float* disparity, const int w, const int h, const float vMin) {
    CHECK(smx_fill_occlusion(disparity, w, h, vMin));
}

// filter.cu:117-207: dead code in the reference (never called from main.cu); a standalone device op here.
void filter(unsigned char* image, int width, int height, unsigned char* mean, float* var, bool) {
    CHECK(smx_filter(&smx_config().params, image, width, height, mean, var));
}

// not in the reference: the weighted-median refinement behind fill_occlusion (smx_main --wmf), default parameters
void weighted_median(unsigned char* guide, float* disparity, float* select, float* out, const int w, const int h,
                     int dmin, int size_d, bool host_gpu_compare) {
    smx_wmf_params p;
    smx_default_wmf_params(&p);
    CHECK(smx_weighted_median(&p, guide, disparity, select, out, w, h, dmin, size_d));
    if (host_gpu_compare) {
        std::vector<float> twin((size_t)w * h);
        weighted_medianOnCPU(guide, disparity, select, twin.data(), w, h, dmin, size_d, p);
        if (check_errors(twin.data(), out, w * h)) cout << "Weighted median ok!" << endl;
    }
}

// not in the reference: speckle removal between the LR check and fill_occlusion (smx_main --speckle)
void speckle_filter(float* disparity, float* out, const int w, const int h, float vmin, float new_val,
                    const smx_speckle_params& p, bool host_gpu_compare) {
    CHECK(smx_speckle_filter(&p, disparity, out, w, h, vmin, new_val));
    if (host_gpu_compare) {
        std::vector<float> twin((size_t)w * h);
        speckle_filterOnCPU(disparity, twin.data(), w, h, vmin, new_val, p);
        if (check_errors(twin.data(), out, w * h)) cout << "Speckle filter ok!" << endl;
    }
}

// not in the reference: region voting and interpolation behind speckle removal (smx_main --vote)
void region_vote(unsigned char* guide, int channels, float* disparity, float* disparity_right, float* out, const int w,
                 const int h, const int dmin, const int size_d, const smx_vote_params& p, const smx_cross_params& arms,
                 bool host_gpu_compare) {
    CHECK(smx_region_vote(&p, &arms, guide, channels, disparity, disparity_right, out, w, h, dmin, size_d,
                          smx_config().params.d_lr));
    if (host_gpu_compare) {
        std::vector<float> twin((size_t)w * h);
        region_voteOnCPU(guide, channels, disparity, disparity_right, twin.data(), w, h, dmin, size_d, p, arms);
        if (check_errors(twin.data(), out, w * h)) cout << "Region voting ok!" << endl;
    }
}

// not in the reference: depth-discontinuity adjustment of a label map from the aggregated costs (smx_main --adjust)
void discontinuity_adjust(float* disparity, float* agg, float* out, const int w, const int h, const int dmin, const int size_d,
                          const smx_adjust_params& p, int subpix_mode, float* sub, bool host_gpu_compare) {
    std::vector<float> ts;
    if (host_gpu_compare && sub) ts.assign(sub, sub + (size_t)w * h);      // (sub is IN/OUT: the twin starts from what the GPU starts from)
    CHECK(smx_discontinuity_adjust(&p, disparity, agg, out, w, h, dmin, size_d, subpix_mode, sub));
    if (host_gpu_compare) {
        std::vector<float> twin((size_t)w * h);
        discontinuityAdjustOnCPU(disparity, agg, twin.data(), w, h, dmin, size_d, p, subpix_mode, sub ? ts.data() : nullptr);
        bool ok = check_errors(twin.data(), out, w * h);
        if (sub) ok = check_errors(ts.data(), sub, w * h) && ok;
        if (ok) cout << "Discontinuity adjustment ok!" << endl;
    }
}

// not in the reference: PatchMatch stereo, a disparity plane per pixel (smx_main --aggregation patchmatch)
void patch_match(unsigned char* left, unsigned char* right, float* planes, float* cost, float* disp, float* label, const int w,
                 const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p, bool host_gpu_compare) {
    CHECK(smx_patchmatch(&smx_config().params, &p, left, right, w, h, size_d, dminl, dminr, planes, cost, disp, label));
    if (host_gpu_compare) {
        const size_t n = (size_t)w * h;
        std::vector<float> tp(6 * n), tc(2 * n), td(2 * n), tl(2 * n);
        patchMatchOnCPU(left, right, tp.data(), tc.data(), td.data(), tl.data(), w, h, size_d, dminl, dminr, p);
        bool ok = check_errors(tp.data(), planes, (int)(6 * n));
        ok = check_errors(tc.data(), cost, (int)(2 * n)) && ok;
        ok = check_errors(td.data(), disp, (int)(2 * n)) && ok;
        ok = check_errors(tl.data(), label, (int)(2 * n)) && ok;
        if (ok) cout << "PatchMatch ok!" << endl;
    }
}

// not in the reference: the information permeability filter of one volume (smx_main --permeability runs it inside the context)
void permeability_filter(float* volume, unsigned char* guide, int channels, float* out, float* best, float* disp_map, const int w,
                         const int h, const int dmin, const int size_d, const smx_perm_params& p, bool host_gpu_compare) {
    CHECK(smx_permeability_filter(&p, volume, guide, channels, w, h, dmin, size_d, out, best, disp_map));
    if (host_gpu_compare) {
        const size_t n = (size_t)w * h;
        std::vector<float> to(n * size_d), tb(n), td(n);
        permeabilityOnCPU(volume, guide, channels, to.data(), tb.data(), td.data(), w, h, dmin, size_d, p);
        bool ok = !out || check_errors(to.data(), out, (int)(n * size_d));
        ok = (!best || check_errors(tb.data(), best, (int)n)) && ok;
        ok = (!disp_map || check_errors(td.data(), disp_map, (int)n)) && ok;
        if (ok) cout << "Permeability ok!" << endl;
    }
}

// not in the reference: the guided filter with a colour guide (smx_main --guidance rgb)
void compute_colour_guided_filter(unsigned char* rgb, int channels, float* cost, float* filter_cost, float* disp_map, float* agg,
                                  const int w, const int h, const int size_d, const int dmin, bool host_gpu_compare) {
    std::vector<float> tb, td;
    if (host_gpu_compare) {            // (filter_cost / disp_map are IN/OUT: the twin starts from what the GPU starts from)
        tb.assign(filter_cost, filter_cost + (size_t)w * h);
        td.assign(disp_map, disp_map + (size_t)w * h);
    }
    CHECK(smx_colour_guided_filter(&smx_config().params, rgb, channels, cost, filter_cost, disp_map, agg, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> ta(agg ? (size_t)w * h * size_d : 0);
        colour_guided_filterOnCPU(rgb, channels, cost, tb.data(), td.data(), agg ? ta.data() : nullptr, w, h, size_d, dmin,
                                  smx_config().params.radius, smx_config().params.eps);
        compare_aggregation("Colour guided filter", tb, td, ta, filter_cost, disp_map, agg, w * h, size_d);
    }
}

// not in the reference: cross-based aggregation instead of the guided filter (smx_main --aggregation cross)
void cross_aggregate(unsigned char* guide, int channels, float* cost, float* filter_cost, float* disp_map, float* agg,
                     const int w, const int h, const int size_d, const int dmin, const smx_cross_params& p, bool host_gpu_compare) {
    std::vector<float> tb, td;
    if (host_gpu_compare) {            // (filter_cost / disp_map are IN/OUT: the twin starts from what the GPU starts from)
        tb.assign(filter_cost, filter_cost + (size_t)w * h);
        td.assign(disp_map, disp_map + (size_t)w * h);
    }
    CHECK(smx_cross_aggregate(&p, guide, channels, cost, filter_cost, disp_map, agg, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> ta(agg ? (size_t)w * h * size_d : 0);
        cross_aggregateOnCPU(guide, channels, cost, tb.data(), td.data(), agg ? ta.data() : nullptr, w, h, size_d, dmin, p);
        compare_aggregation("Cross-based aggregation", tb, td, ta, filter_cost, disp_map, agg, w * h, size_d);
    }
}

// not in the reference: semi-global matching instead of the guided filter (smx_main --aggregation sgm)
void sgm_aggregate(float* cost, float* agg, float* best, float* disp_map, const int w, const int h, const int size_d,
                   const int dmin, const smx_sgm_params& p, bool host_gpu_compare) {
    CHECK(smx_sgm_aggregate(&p, cost, agg, best, disp_map, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> tb((size_t)w * h), td((size_t)w * h), ta(agg ? (size_t)w * h * size_d : 0);
        sgm_aggregateOnCPU(cost, agg ? ta.data() : nullptr, tb.data(), td.data(), w, h, size_d, dmin, p);
        compare_aggregation("Semi-global matching", tb, td, ta, best, disp_map, agg, w * h, size_d);
    }
}

// not in the reference: hierarchical belief propagation instead of the guided filter (smx_main --aggregation bp)
void belief_propagation(float* cost, float* agg, float* best, float* disp_map, const int w, const int h, const int size_d,
                        const int dmin, const smx_bp_params& p, bool host_gpu_compare) {
    CHECK(smx_bp_aggregate(&p, cost, agg, best, disp_map, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> tb((size_t)w * h), td((size_t)w * h), ta(agg ? (size_t)w * h * size_d : 0);
        beliefPropagationOnCPU(cost, agg ? ta.data() : nullptr, tb.data(), td.data(), w, h, size_d, dmin, p);
        compare_aggregation("Belief propagation", tb, td, ta, best, disp_map, agg, w * h, size_d);
    }
}

// not in the reference: the scan-line optimiser with colour-adaptive penalties (smx_main --aggregation scanline / cross-scanline)
void scanline_optimize(unsigned char* guide_own, unsigned char* guide_other, int channels, float* cost, float* agg, float* best,
                       float* disp_map, const int w, const int h, const int size_d, const int dmin, const smx_scanline_params& p,
                       bool host_gpu_compare) {
    CHECK(smx_scanline_optimize(&p, guide_own, guide_other, channels, cost, agg, best, disp_map, w, h, size_d, dmin));
    if (host_gpu_compare) {
        std::vector<float> tb((size_t)w * h), td((size_t)w * h), ta(agg ? (size_t)w * h * size_d : 0);
        scanline_optimizeOnCPU(guide_own, guide_other, channels, cost, agg ? ta.data() : nullptr, tb.data(), td.data(), w, h, size_d,
                               dmin, p);
        compare_aggregation("Scan-line optimisation", tb, td, ta, best, disp_map, agg, w * h, size_d);
    }
}
