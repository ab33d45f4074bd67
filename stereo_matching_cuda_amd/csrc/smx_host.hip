// smx_host.hip -- the host-pointer stage entries of include/smx.h (the reference's L2 wrappers).  Each reads as: its argument
// checks, its inputs, the device entry of smx_capi.hip, the synchronise, its outputs.
#include <limits.h>

#include <vector>

#include "smx_api.h"
#include "smx_launch.h"

using namespace smx;

// every slice in flight, but at most ~2 GiB of them; bytes(k): a stage's workspace for k slices in flight
template <class Bytes> static size_t capped_ws_bytes(Bytes bytes, int size_d) {
    const size_t one = bytes(1), all = bytes(size_d), cap = (size_t)2 << 30;
    return all <= cap ? all : one > cap ? one : cap;
}

size_t smx::pick_ws_bytes(int w, int h, int size_d) {
    return capped_ws_bytes([=](int k) { return smx_agg_workspace_bytes(w, h, k); }, size_d);
}

// The body of smx_colour_guided_filter and smx_cross_aggregate behind their argument checks: guide, cost and the caller's
// presets up; fresh keys; entry(guide, cost, keys, agg, ws): the stage's one-view device entry; the keys onto the presets; down.
template <class Entry>
static int guide_aggregate_host(const uint8_t* guide, int channels, const float* cost, float* filter_cost, float* disp_map,
                                float* agg, int w, int h, int size_d, int dmin, size_t ws_bytes, Entry entry) {
    const size_t n = (size_t)w * h, fb = n * sizeof(float), vb = fb * size_d;
    DevBuf dI, dC, dBest, dMap, dKeys, dAgg, ws;
    SMX_HIP(dI.upload(guide, n * channels));
    SMX_HIP(dC.upload(cost, vb));
    SMX_HIP(dBest.upload(filter_cost, fb));
    SMX_HIP(dMap.upload(disp_map, fb));
    SMX_HIP(dKeys.ensure(n * sizeof(int64_t)));
    if (agg) SMX_HIP(dAgg.ensure(vb));
    SMX_HIP(ws.ensure(ws_bytes));
    int rc;
    if ((rc = smx_dev_init_keys(dKeys.as<int64_t>(), (int64_t)n, nullptr))) return rc;
    if ((rc = entry(dI.as<uint8_t>(), dC.as<float>(), dKeys.as<int64_t>(), agg ? dAgg.as<float>() : nullptr, ws.p))) return rc;
    if ((rc = smx_dev_apply_keys(dKeys.as<int64_t>(), (int64_t)n, dmin, dBest.as<float>(), dMap.as<float>(), nullptr))) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dBest.download(filter_cost, fb));
    SMX_HIP(dMap.download(disp_map, fb));
    if (agg) SMX_HIP(dAgg.download(agg, vb));
    return SMX_OK;
}

extern "C" {

int smx_rgb_to_grayscale(const smx_params* p, const uint8_t* h_rgb, int64_t n, int channels, uint8_t* h_gray) {
    SMX_ARG(p && h_rgb && h_gray && n > 0 && channels >= 3);
    DevBuf rgb, gray;
    SMX_HIP(rgb.upload(h_rgb, (size_t)n * channels));
    SMX_HIP(gray.ensure((size_t)n));
    if (int rc = smx_dev_rgb_to_grayscale(p, rgb.as<uint8_t>(), n, channels, gray.as<uint8_t>(), nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(gray.download(h_gray, (size_t)n));
    return SMX_OK;
}

int smx_compute_cost(const smx_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w1, int w2, int h1, int h2,
                     int size_d, int dmin) {
    SMX_ARG(p && i1 && i2 && cost && size_d >= 1);
    SMX_ARG(w1 >= 2 && w1 == w2 && h1 >= 1 && h1 == h2);
    const size_t n = (size_t)w1 * h1;
    DevBuf d1, d2, dc;
    SMX_HIP(d1.upload(i1, n));
    SMX_HIP(d2.upload(i2, n));
    SMX_HIP(dc.ensure(n * size_d * sizeof(float)));
    if (int rc = smx_dev_cost_volume(p, d1.as<uint8_t>(), d2.as<uint8_t>(), dc.as<float>(), w1, w2, h1, dmin, 0, size_d, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dc.download(cost, n * size_d * sizeof(float)));
    return SMX_OK;
}

int smx_integral(const float* image, float* integral, int width, int height) {
    SMX_ARG(image && integral && width >= 1 && height >= 1);
    const size_t bytes = (size_t)width * height * sizeof(float);
    DevBuf d;
    SMX_HIP(d.upload(image, bytes));
    if (int rc = smx_dev_integral(d.as<float>(), d.as<float>(), width, height, 1, nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(d.download(integral, bytes));
    return SMX_OK;
}

int smx_compute_guided_filter(const smx_params* p, const uint8_t* i, const float* cost, float* filter_cost, float* disp_map,
                              uint8_t* mean, float* agg, int w, int h, int size_d, int dmin) {
    SMX_ARG(p && i && cost && filter_cost && disp_map && size_d >= 1 && w >= 2 && h >= 1);
    const size_t n = (size_t)w * h, fb = n * sizeof(float), vb = fb * size_d;
    const size_t ws_bytes = pick_ws_bytes(w, h, size_d);
    DevBuf dI, dC, dBest, dMap, dMean, dKeys, dAgg, ws;
    SMX_HIP(dI.upload(i, n));
    SMX_HIP(dC.upload(cost, vb));
    SMX_HIP(dBest.upload(filter_cost, fb));
    SMX_HIP(dMap.upload(disp_map, fb));
    SMX_HIP(dMean.ensure(n));
    SMX_HIP(dKeys.ensure(n * sizeof(int64_t)));
    if (agg) SMX_HIP(dAgg.ensure(vb));
    SMX_HIP(ws.ensure(ws_bytes));
    int rc;
    if ((rc = smx_dev_init_keys(dKeys.as<int64_t>(), (int64_t)n, nullptr))) return rc;
    if ((rc = smx_dev_aggregate_wta(p, dI.as<uint8_t>(), nullptr, dC.as<float>(), w, h, dmin, 0, size_d, dKeys.as<int64_t>(),
                                    dMean.as<uint8_t>(), agg ? dAgg.as<float>() : nullptr, ws.p, ws_bytes, nullptr)))
        return rc;
    if ((rc = smx_dev_apply_keys(dKeys.as<int64_t>(), (int64_t)n, dmin, dBest.as<float>(), dMap.as<float>(), nullptr))) return rc;
    SMX_HIP(hipDeviceSynchronize());
    if ((rc = smx_dev_agg_status(ws.p))) return rc;
    SMX_HIP(dBest.download(filter_cost, fb));
    SMX_HIP(dMap.download(disp_map, fb));
    if (mean) SMX_HIP(dMean.download(mean, n));
    if (agg) SMX_HIP(dAgg.download(agg, vb));
    return SMX_OK;
}

int smx_detect_occlusion(const smx_params* p, float* disparityLeft, const float* disparityRight, int dOcclusion, int w, int h) {
    SMX_ARG(p && disparityLeft && disparityRight && w >= 1 && h >= 1);
    const size_t bytes = (size_t)w * h * sizeof(float);
    DevBuf dL, dR;
    SMX_HIP(dL.upload(disparityLeft, bytes));
    SMX_HIP(dR.upload(disparityRight, bytes));
    if (int rc = smx_dev_detect_occlusion(p, dL.as<float>(), dR.as<float>(), dOcclusion, w, h, nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dL.download(disparityLeft, bytes));
    return SMX_OK;
}

int smx_fill_occlusion(float* disparity, int w, int h, float vMin) {
    SMX_ARG(disparity && w >= 1 && h >= 1);
    const size_t bytes = (size_t)w * h * sizeof(float);
    DevBuf d;
    SMX_HIP(d.upload(disparity, bytes));
    if (int rc = smx_dev_fill_occlusion(d.as<float>(), w, h, vMin, nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(d.download(disparity, bytes));
    return SMX_OK;
}

int smx_weighted_median(const smx_wmf_params* p, const uint8_t* guide, const float* disp, const float* select, float* out, int w,
                        int h, int dmin, int size_d) {
    SMX_ARG(wmf_params_ok(p) && guide && disp && out && w >= 1 && h >= 1);
    SMX_ARG(size_d >= 1 && size_d <= 4096 && (long long)dmin + size_d <= INT_MAX);
    SMX_ARG((const void*)out != (const void*)disp);
    const size_t n = (size_t)w * h, bytes = n * sizeof(float);
    DevBuf dG, dD, dS, dO;
    SMX_HIP(dG.upload(guide, n));
    SMX_HIP(dD.upload(disp, bytes));
    SMX_HIP(dO.ensure(bytes));
    if (select) SMX_HIP(dS.upload(select, bytes));
    if (int rc = smx_dev_weighted_median(p, dG.as<uint8_t>(), dD.as<float>(), select ? dS.as<float>() : nullptr, dO.as<float>(),
                                         w, h, dmin, size_d, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dO.download(out, bytes));
    return SMX_OK;
}

int smx_speckle_filter(const smx_speckle_params* p, const float* disp, float* out, int w, int h, float vmin, float new_val) {
    SMX_ARG(speckle_params_ok(p) && disp && out && shape_ok(w, h, 1, 1));
    const size_t bytes = (size_t)w * h * sizeof(float), wsb = speckle_workspace_bytes(w, h);
    DevBuf dD, dW;
    SMX_HIP(dD.upload(disp, bytes));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_speckle_filter(p, dD.as<float>(), dD.as<float>(), w, h, vmin, new_val, dW.p, wsb, nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dD.download(out, bytes));
    return SMX_OK;
}

int smx_uniqueness_filter(float ratio, const int64_t* keys, const float* uq, const float* disp, float* out, float* margin, int w,
                          int h, float vmin, float new_val) {
    SMX_ARG(uniq_ratio_ok(ratio));
    SMX_ARG(keys && uq && disp && out && w >= 1 && h >= 1);
    const size_t n = (size_t)w * h, bytes = n * sizeof(float);
    DevBuf dK, dU, dD, dM;
    SMX_HIP(dK.upload(keys, n * sizeof(int64_t)));
    SMX_HIP(dU.upload(uq, bytes));                    // (the test reads the sec plane only)
    SMX_HIP(dD.upload(disp, bytes));
    if (margin) SMX_HIP(dM.ensure(bytes));
    if (int rc = smx_dev_uniqueness(ratio, dK.as<int64_t>(), dU.as<float>(), dD.as<float>(), dD.as<float>(),
                                    margin ? dM.as<float>() : nullptr, w, h, vmin, new_val, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dD.download(out, bytes));
    if (margin) SMX_HIP(dM.download(margin, bytes));
    return SMX_OK;
}

int smx_census_cost(const smx_census_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h,
                    int size_d, int dmin) {
    SMX_ARG(census_params_ok(p) && i1 && i2 && cost && w >= 1 && h >= 1 && size_d >= 1);
    const size_t n = (size_t)w * h;
    DevBuf img, code, dc;
    SMX_HIP(img.ensure(2 * n));
    SMX_HIP(code.ensure(2 * n * sizeof(uint64_t)));
    SMX_HIP(dc.ensure(n * size_d * sizeof(float)));
    SMX_HIP(hipMemcpy(img.p, i1, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + n, i2, n, hipMemcpyHostToDevice));
    int rc;
    if ((rc = smx_dev_census(p, img.as<uint8_t>(), code.as<uint64_t>(), w, h, 2, nullptr))) return rc;
    if ((rc = smx_dev_census_cost_pair(p, code.as<uint64_t>(), dc.as<float>(), nullptr, w, h, dmin, 0, 0, size_d, nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dc.download(cost, n * size_d * sizeof(float)));
    return SMX_OK;
}

int smx_zncc_cost(const smx_zncc_params* p, const uint8_t* i1, const uint8_t* i2, float* cost, int w, int h, int size_d,
                  int dmin) {
    if (!zncc_params_ok(p)) return fail(SMX_E_ARG, "smx_zncc_cost: %s", ZNCC_RANGES);
    SMX_ARG(i1 && i2 && cost && w >= 1 && h >= 1 && size_d >= 1);
    const size_t n = (size_t)w * h;
    DevBuf img, mom, dc;
    SMX_HIP(img.ensure(2 * n));
    SMX_HIP(mom.ensure(2 * n * sizeof(uint64_t)));
    SMX_HIP(dc.ensure(n * size_d * sizeof(float)));
    SMX_HIP(hipMemcpy(img.p, i1, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + n, i2, n, hipMemcpyHostToDevice));
    int rc;
    if ((rc = smx_dev_zncc_moments(p, img.as<uint8_t>(), mom.as<uint64_t>(), w, h, 2, nullptr))) return rc;
    if ((rc = smx_dev_zncc_cost_pair(p, mom.as<uint64_t>(), img.as<uint8_t>(), img.as<uint8_t>() + n, dc.as<float>(), nullptr, w, h, dmin, 0, 0,
                                     size_d, nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dc.download(cost, n * size_d * sizeof(float)));
    return SMX_OK;
}

int smx_adcensus_cost(const smx_adcensus_params* p, const uint8_t* i1, const uint8_t* i2, int channels, float* cost, int w,
                      int h, int size_d, int dmin) {
    SMX_ARG(adcensus_params_ok(p) && i1 && i2 && cost && w >= 1 && h >= 1 && size_d >= 1);
    SMX_ARG(p->colour ? channels == 3 || channels == 4 : channels == 1);
    const size_t n = (size_t)w * h, ib = n * (size_t)channels;
    DevBuf img, gray, code, tab, dc;
    SMX_HIP(img.ensure(2 * ib));
    SMX_HIP(code.ensure(2 * n * sizeof(uint64_t)));
    SMX_HIP(tab.ensure(SMX_ADCENSUS_TABLE_FLOATS * sizeof(float)));
    SMX_HIP(dc.ensure(n * size_d * sizeof(float)));
    SMX_HIP(hipMemcpy(img.p, i1, ib, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + ib, i2, ib, hipMemcpyHostToDevice));
    int rc;
    const uint8_t* g = img.as<uint8_t>();
    if (p->colour) {          // the codes come from the gray images
        smx_params dp;
        smx_default_params(&dp);
        SMX_HIP(gray.ensure(2 * n));
        if ((rc = smx_dev_rgb_to_grayscale(&dp, img.as<uint8_t>(), (int64_t)(2 * n), channels, gray.as<uint8_t>(), nullptr))) return rc;
        g = gray.as<uint8_t>();
    }
    if ((rc = smx_dev_adcensus_tables(p, tab.as<float>(), nullptr))) return rc;
    if ((rc = smx_dev_census(&p->census, g, code.as<uint64_t>(), w, h, 2, nullptr))) return rc;
    if ((rc = smx_dev_adcensus_cost_pair(p, tab.as<float>(), code.as<uint64_t>(), img.as<uint8_t>(), img.as<uint8_t>() + ib, channels,
                                         dc.as<float>(), nullptr, w, h, dmin, 0, 0, size_d, nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dc.download(cost, n * size_d * sizeof(float)));
    return SMX_OK;
}

int smx_mi_histogram(const uint8_t* img_l, const uint8_t* img_r, const float* map, float occlusion_mark, uint32_t* hist,
                     int w, int h) {
    SMX_ARG(img_l && img_r && map && hist);
    if (!shape_ok(w, h, 1, 1)) return fail(SMX_E_ARG, "smx_mi_histogram: %s", PLANE_SHAPES);
    const size_t n = (size_t)w * h, hb = (size_t)SMX_MI_LEVELS * SMX_MI_LEVELS * sizeof(uint32_t);
    DevBuf img, dm, dh;
    SMX_HIP(img.ensure(2 * n));
    SMX_HIP(dh.ensure(hb));
    SMX_HIP(hipMemcpy(img.p, img_l, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + n, img_r, n, hipMemcpyHostToDevice));
    SMX_HIP(dm.upload(map, n * sizeof(float)));
    if (int rc = smx_dev_mi_histogram(img.as<uint8_t>(), img.as<uint8_t>() + n, dm.as<float>(), occlusion_mark, dh.as<uint32_t>(),
                                      w, h, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dh.download(hist, hb));
    return SMX_OK;
}

int smx_mi_cost(const uint8_t* table, const uint8_t* i1, const uint8_t* i2, int right, float* cost, int w, int h, int size_d,
                int dmin) {
    SMX_ARG(table && i1 && i2 && cost && (right == 0 || right == 1) && w >= 1 && h >= 1 && size_d >= 1);
    const size_t n = (size_t)w * h;
    DevBuf img, tab, dc;
    SMX_HIP(img.ensure(2 * n));
    SMX_HIP(tab.upload(table, (size_t)SMX_MI_LEVELS * SMX_MI_LEVELS));
    SMX_HIP(dc.ensure(n * size_d * sizeof(float)));
    // (the left image first, whichever view is asked for)
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + (right ? n : 0), i1, n, hipMemcpyHostToDevice));
    SMX_HIP(hipMemcpy(img.as<uint8_t>() + (right ? 0 : n), i2, n, hipMemcpyHostToDevice));
    if (int rc = smx_dev_mi_cost_pair(tab.as<uint8_t>(), img.as<uint8_t>(), img.as<uint8_t>() + n, right ? nullptr : dc.as<float>(),
                                      right ? dc.as<float>() : nullptr, w, h, dmin, dmin, 0, size_d, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dc.download(cost, n * size_d * sizeof(float)));
    return SMX_OK;
}

int smx_sgm_aggregate(const smx_sgm_params* p, const float* cost, float* agg, float* best, float* disp_map, int w, int h,
                      int size_d, int dmin) {
    if (!sgm_params_ok(p)) return fail(SMX_E_ARG, "smx_sgm_aggregate: %s", SGM_RANGES);
    if (!shape_ok(w, h, size_d, SMX_SGM_MAX_D)) return fail(SMX_E_ARG, "smx_sgm_aggregate: %s", SGM_SHAPES);
    SMX_ARG(cost != nullptr);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float), wsb = sgm_workspace_bytes(w, h, size_d, 1);
    DevBuf dC, dA, dK, dW;
    SMX_HIP(dC.upload(cost, vb));
    if (agg) SMX_HIP(dA.ensure(vb));
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_sgm_wta_pair(p, dC.as<float>(), nullptr, w, h, size_d, dK.as<int64_t>(), agg ? dA.as<float>() : nullptr,
                                      nullptr, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (agg) SMX_HIP(dA.download(agg, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_bp_aggregate(const smx_bp_params* p, const float* cost, float* agg, float* best, float* disp_map, int w, int h, int size_d,
                     int dmin) {
    if (!bp_params_ok(p)) return fail(SMX_E_ARG, "smx_bp_aggregate: %s", BP_RANGES);
    if (!shape_ok(w, h, size_d, SMX_BP_MAX_D)) return fail(SMX_E_ARG, "smx_bp_aggregate: %s", BP_SHAPES);
    SMX_ARG(cost != nullptr);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float), wsb = bp_workspace_bytes(w, h, size_d, p->levels, 1);
    DevBuf dC, dA, dK, dW;
    SMX_HIP(dC.upload(cost, vb));
    if (agg) SMX_HIP(dA.ensure(vb));
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_bp_wta_pair(p, dC.as<float>(), nullptr, w, h, size_d, dK.as<int64_t>(), agg ? dA.as<float>() : nullptr,
                                     nullptr, nullptr, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (agg) SMX_HIP(dA.download(agg, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_scanline_optimize(const smx_scanline_params* p, const uint8_t* guide_own, const uint8_t* guide_other, int channels,
                          const float* cost, float* agg, float* best, float* disp_map, int w, int h, int size_d, int dmin) {
    if (!scanline_params_ok(p)) return fail(SMX_E_ARG, "smx_scanline_optimize: %s", SCANLINE_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, SMX_SGM_MAX_D)) return fail(SMX_E_ARG, "smx_scanline_optimize: %s", SGM_SHAPES);
    SMX_ARG(guide_own && guide_other && cost);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float), wsb = scanline_workspace_bytes(w, h, size_d, 1);
    DevBuf dG, dH, dC, dA, dK, dW;
    SMX_HIP(dG.upload(guide_own, n * channels));
    SMX_HIP(dH.upload(guide_other, n * channels));
    SMX_HIP(dC.upload(cost, vb));
    if (agg) SMX_HIP(dA.ensure(vb));
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    SMX_HIP(dW.ensure(wsb));
    // the one view goes in as the left one: its partners lie in `guide_other`
    if (int rc = smx_dev_scanline_wta_pair(p, dG.as<uint8_t>(), dH.as<uint8_t>(), channels, dC.as<float>(), nullptr, w, h, size_d,
                                           dmin, 0, dK.as<int64_t>(), agg ? dA.as<float>() : nullptr, nullptr, nullptr, dW.p,
                                           wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (agg) SMX_HIP(dA.download(agg, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_colour_guided_filter(const smx_params* p, const uint8_t* rgb, int channels, const float* cost, float* filter_cost,
                             float* disp_map, float* agg, int w, int h, int size_d, int dmin) {
    SMX_ARG(p && rgb && cost && filter_cost && disp_map && size_d >= 1 && w >= 1 && h >= 1);
    SMX_ARG(p->radius >= 0 && (channels == 3 || channels == 4));
    const size_t one = smx_cgf_workspace_bytes(w, h, 1, 1);
    SMX_ARG(one != 0);
    const size_t ws_bytes = capped_ws_bytes([=](int k) { return cgf_workspace_bytes(w, h, k, 1); }, size_d);
    return guide_aggregate_host(rgb, channels, cost, filter_cost, disp_map, agg, w, h, size_d, dmin, ws_bytes,
                                [=](const uint8_t* d_rgb, const float* d_cost, int64_t* d_keys, float* d_agg, void* d_ws) {
                                    return smx_dev_cgf_wta_pair(p, d_rgb, nullptr, channels, d_cost, nullptr, w, h, 0, size_d, d_keys,
                                                                d_agg, nullptr, nullptr, d_ws, ws_bytes, nullptr);
                                });
}

int smx_cross_aggregate(const smx_cross_params* p, const uint8_t* guide, int channels, const float* cost, float* filter_cost,
                        float* disp_map, float* agg, int w, int h, int size_d, int dmin) {
    if (!cross_params_ok(p)) return fail(SMX_E_ARG, "smx_cross_aggregate: %s", CROSS_RANGES);
    SMX_ARG(guide && cost && filter_cost && disp_map && size_d >= 1);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, 1, 1)) return fail(SMX_E_ARG, "smx_cross_aggregate: %s", PLANE_SHAPES);
    const size_t ws_bytes = capped_ws_bytes([=](int k) { return cross_workspace_bytes(w, h, k, 1); }, size_d);
    return guide_aggregate_host(guide, channels, cost, filter_cost, disp_map, agg, w, h, size_d, dmin, ws_bytes,
                                [=](const uint8_t* d_guide, const float* d_cost, int64_t* d_keys, float* d_agg, void* d_ws) {
                                    return smx_dev_cross_wta_pair(p, d_guide, nullptr, channels, d_cost, nullptr, w, h, 0, size_d,
                                                                  d_keys, d_agg, nullptr, nullptr, d_ws, ws_bytes, nullptr);
                                });
}

int smx_region_vote(const smx_vote_params* p, const smx_cross_params* cross, const uint8_t* guide, int channels, const float* disp,
                    const float* disp_r, float* out, int w, int h, int dmin, int size_d, int d_lr) {
    if (!vote_params_ok(p)) return fail(SMX_E_ARG, "smx_region_vote: %s", VOTE_RANGES);
    smx_cross_params cp;
    smx_default_cross_params(&cp);
    if (cross) { cp = *cross; cp.iterations = 1; }
    if (!cross_params_ok(&cp)) return fail(SMX_E_ARG, "smx_region_vote: the arms: %s", CROSS_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, VOTE_MAX_D)) return fail(SMX_E_ARG, "smx_region_vote: %s", VOTE_SHAPES);
    SMX_ARG(guide && disp && out);
    const size_t n = (size_t)w * h, fb = n * sizeof(float), wsb = vote_workspace_bytes(w, h);
    DevBuf dG, dA, dD, dR, dW;
    SMX_HIP(dG.upload(guide, n * channels));
    SMX_HIP(dA.ensure(n * sizeof(uint32_t)));
    SMX_HIP(dD.upload(disp, fb));
    if (disp_r) SMX_HIP(dR.upload(disp_r, fb));
    SMX_HIP(dW.ensure(wsb));
    int rc;
    if ((rc = smx_dev_cross_arms(&cp, dG.as<uint8_t>(), nullptr, channels, w, h, dA.as<uint32_t>(), nullptr))) return rc;
    if ((rc = smx_dev_region_vote(p, dA.as<uint32_t>(), dG.as<uint8_t>(), channels, dD.as<float>(), disp_r ? dR.as<float>() : nullptr,
                                  dD.as<float>(), w, h, dmin, size_d, d_lr, dW.p, wsb, nullptr)))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dD.download(out, fb));
    return SMX_OK;
}

int smx_discontinuity_adjust(const smx_adjust_params* p, const float* disp, const float* agg, float* out, int w, int h, int dmin,
                             int size_d, int subpix_mode, float* sub) {
    if (!adjust_params_ok(p)) return fail(SMX_E_ARG, "smx_discontinuity_adjust: %s", ADJUST_RANGES);
    if (!shape_ok(w, h, size_d, ADJ_MAX_D)) return fail(SMX_E_ARG, "smx_discontinuity_adjust: %s", ADJUST_SHAPES);
    SMX_ARG(disp && agg && out);
    if (sub ? !subpix_mode_ok(subpix_mode) : subpix_mode != 0 && !subpix_mode_ok(subpix_mode))
        return fail(SMX_E_ARG, "smx_discontinuity_adjust: subpix_mode must be SMX_SUBPIX_PARABOLA or SMX_SUBPIX_EQUIANGULAR (or 0 "
                               "without sub)");
    const size_t n = (size_t)w * h, fb = n * sizeof(float), wsb = adjust_workspace_bytes(w, h);
    DevBuf dD, dA, dS, dW;
    SMX_HIP(dD.upload(disp, fb));
    SMX_HIP(dA.upload(agg, fb * size_d));
    if (sub) SMX_HIP(dS.upload(sub, fb));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_discontinuity_adjust(p, dD.as<float>(), dA.as<float>(), dD.as<float>(), w, h, dmin, size_d, subpix_mode,
                                              sub ? dS.as<float>() : nullptr, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dD.download(out, fb));
    if (sub) SMX_HIP(dS.download(sub, fb));
    return SMX_OK;
}

int smx_pyr_down(const uint8_t* src, uint8_t* dst, int w, int h, int channels) {
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, 1, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_pyr_down: %s", PLANE_SHAPES);
    SMX_ARG(src && dst);
    const size_t in = (size_t)w * h * channels, out = (size_t)((w + 1) / 2) * ((h + 1) / 2) * channels;
    DevBuf dS, dD;
    SMX_HIP(dS.upload(src, in));
    SMX_HIP(dD.ensure(out));
    if (int rc = smx_dev_pyr_down(dS.as<uint8_t>(), dD.as<uint8_t>(), w, h, channels, nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dD.download(dst, out));
    return SMX_OK;
}

int smx_cscale_combine(const smx_cscale_params* p, const float* const* agg, int w, int h, int dmin, int size_d, float* out,
                       float* best, float* disp_map) {
    if (!cscale_params_ok(p)) return fail(SMX_E_ARG, "smx_cscale_combine: %s", CSCALE_RANGES);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_cscale_combine: %s", CSCALE_SHAPES);
    SMX_ARG(agg != nullptr);
    for (int s = 0; s < p->scales; ++s) SMX_ARG(agg[s] != nullptr);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float);
    DevBuf dA[SMX_CSCALE_MAX_SCALES], dK;
    const float* levels[SMX_CSCALE_MAX_SCALES] = {};
    for (int s = 0; s < p->scales; ++s) {
        int ws, hs, d0, ds;
        cscale_level(w, h, dmin, size_d, s, &ws, &hs, &d0, &ds);
        SMX_HIP(dA[s].upload(agg[s], (size_t)ws * hs * ds * sizeof(float)));
        levels[s] = dA[s].as<float>();
    }
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    // (the combined volume goes over the uploaded level 0)
    if (int rc = smx_dev_cscale_wta_pair(p, levels, nullptr, w, h, dmin, 0, size_d, dK.as<int64_t>(), out ? dA[0].as<float>() : nullptr,
                                         nullptr, nullptr, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (out) SMX_HIP(dA[0].download(out, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_patchmatch(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h, int size_d,
                   int dminl, int dminr, float* planes, float* cost, float* disp, float* label) {
    if (!pm_params_ok(pm)) return fail(SMX_E_ARG, "smx_patchmatch: %s", PM_RANGES);
    if (!pm_shape_ok(w, h, size_d, dminl, dminr)) return fail(SMX_E_ARG, "smx_patchmatch: %s", PM_SHAPES);
    SMX_ARG(p && left && right && planes && cost && disp && label);
    const size_t n = (size_t)w * h, fb = n * sizeof(float), wsb = pm_workspace_bytes(w, h);
    DevBuf dL, dR, dO, dW;                       // dO: planes | cost | disp | label
    SMX_HIP(dL.upload(left, n));
    SMX_HIP(dR.upload(right, n));
    SMX_HIP(dO.ensure(12 * fb));
    SMX_HIP(dW.ensure(wsb));
    float* o = dO.as<float>();
    if (int rc = smx_dev_patchmatch_pair(p, pm, dL.as<uint8_t>(), dR.as<uint8_t>(), w, h, size_d, dminl, dminr, o, o + 6 * n, o + 8 * n,
                                         o + 10 * n, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(hipMemcpy(planes, o, 6 * fb, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(cost, o + 6 * n, 2 * fb, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(disp, o + 8 * n, 2 * fb, hipMemcpyDeviceToHost));
    SMX_HIP(hipMemcpy(label, o + 10 * n, 2 * fb, hipMemcpyDeviceToHost));
    return SMX_OK;
}

int smx_pm_plane_cost(const smx_params* p, const smx_pm_params* pm, const uint8_t* left, const uint8_t* right, int w, int h,
                      int size_d, int dminl, int dminr, const float* planes, float* cost) {
    if (!pm_params_ok(pm)) return fail(SMX_E_ARG, "smx_pm_plane_cost: %s", PM_RANGES);
    if (!pm_shape_ok(w, h, size_d, dminl, dminr)) return fail(SMX_E_ARG, "smx_pm_plane_cost: %s", PM_SHAPES);
    SMX_ARG(p && left && right && planes && cost);
    const size_t n = (size_t)w * h, fb = n * sizeof(float), wsb = pm_workspace_bytes(w, h);
    DevBuf dL, dR, dP, dC, dW;
    SMX_HIP(dL.upload(left, n));
    SMX_HIP(dR.upload(right, n));
    SMX_HIP(dP.upload(planes, 6 * fb));
    SMX_HIP(dC.ensure(2 * fb));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_pm_plane_cost(p, pm, dL.as<uint8_t>(), dR.as<uint8_t>(), w, h, size_d, dminl, dminr, dP.as<float>(),
                                       dC.as<float>(), dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dC.download(cost, 2 * fb));
    return SMX_OK;
}

int smx_permeability_filter(const smx_perm_params* p, const float* volume, const uint8_t* guide, int channels, int w, int h, int dmin,
                            int size_d, float* out, float* best, float* disp_map) {
    if (!perm_params_ok(p)) return fail(SMX_E_ARG, "smx_permeability_filter: %s", PERM_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_permeability_filter: %s", PERM_SHAPES);
    SMX_ARG(volume && guide);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float);
    // (the filtered volume goes over the uploaded one; the workspace: every slice at once up to ~1 GiB, one slice at least)
    size_t wsb = perm_workspace_bytes(w, h, size_d, 1);
    const size_t cap = (size_t)1 << 30, least = perm_workspace_bytes(w, h, 1, 1);
    if (wsb > cap) wsb = cap > least ? cap : least;
    DevBuf dV, dG, dK, dW;
    SMX_HIP(dV.upload(volume, vb));
    SMX_HIP(dG.upload(guide, n * channels));
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_permeability_wta_pair(p, dV.as<float>(), nullptr, dG.as<uint8_t>(), nullptr, channels, w, h, dmin, 0, size_d,
                                               dK.as<int64_t>(), dV.as<float>(), nullptr, nullptr, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (out) SMX_HIP(dV.download(out, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_tree_filter(const smx_tree_params* p, const float* volume, const uint8_t* guide, int channels, int w, int h, int dmin,
                    int size_d, float* out, float* best, float* disp_map) {
    if (!tree_params_ok(p)) return fail(SMX_E_ARG, "smx_tree_filter: %s", TREE_RANGES);
    SMX_ARG(channels == 1 || channels == 3 || channels == 4);
    if (!shape_ok(w, h, size_d, WIDE_MAX_D)) return fail(SMX_E_ARG, "smx_tree_filter: %s", PERM_SHAPES);
    SMX_ARG(volume && guide);
    const size_t n = (size_t)w * h, vb = n * size_d * sizeof(float), tb = smx_tree_bytes(w, h);
    // (the filtered volume goes over the uploaded one; the workspace: every slice at once up to ~1 GiB, one slice at least)
    size_t wsb = tree_workspace_bytes(w, h, size_d, 1) / 2;
    const size_t cap = (size_t)1 << 30, least = n * sizeof(float);
    if (wsb > cap) wsb = cap / least > 1 ? cap / least * least : least;
    std::vector<uint32_t> blob;
    try {
        blob.resize(tb / 4);
    } catch (const std::bad_alloc&) {
        return fail(SMX_E_HIP, "smx_tree_filter: out of host memory");
    }
    if (int rc = smx_tree_build(guide, channels, w, h, blob.data())) return rc;
    DevBuf dV, dT, dK, dW;
    SMX_HIP(dV.upload(volume, vb));
    SMX_HIP(dT.upload(blob.data(), tb));
    SMX_HIP(dK.ensure(n * sizeof(int64_t)));
    SMX_HIP(dW.ensure(wsb));
    if (int rc = smx_dev_tree_wta_pair(p, dV.as<float>(), nullptr, dT.p, nullptr, w, h, dmin, 0, size_d, dK.as<int64_t>(), dV.as<float>(),
                                       nullptr, nullptr, dW.p, wsb, nullptr))
        return rc;
    SMX_HIP(hipDeviceSynchronize());
    if (out) SMX_HIP(dV.download(out, vb));
    if (best || disp_map) {
        std::vector<int64_t> keys(n);
        SMX_HIP(dK.download(keys.data(), n * sizeof(int64_t)));
        for (size_t i = 0; i < n; ++i) {
            float c; uint32_t z;
            unpack_key(keys[i], &c, &z);
            if (best) best[i] = c;
            if (disp_map) disp_map[i] = (float)(dmin + (int)z);
        }
    }
    return SMX_OK;
}

int smx_filter(const smx_params* p, const uint8_t* image, int w, int h, uint8_t* mean, float* var) {
    SMX_ARG(p && image && mean && var && w >= 1 && h >= 1 && p->radius >= 0);
    const size_t n = (size_t)w * h;
    DevBuf dI, dM, dV;
    SMX_HIP(dI.upload(image, n));
    SMX_HIP(dM.ensure(n));
    SMX_HIP(dV.ensure(n * sizeof(float)));
    if (int rc = smx_dev_filter(p, dI.as<uint8_t>(), w, h, dM.as<uint8_t>(), dV.as<float>(), nullptr)) return rc;
    SMX_HIP(hipDeviceSynchronize());
    SMX_HIP(dM.download(mean, n));
    SMX_HIP(dV.download(var, n * sizeof(float)));
    return SMX_OK;
}

}  // extern "C"
