// cpu_twins.cpp -- host-side twins of the device stages for the `host_gpu_compare` self-check mode of the
// reference (main.cu:40, costVolume.cu:56-74, rgb_to_grayscale.cu:60-65, guidedFilter.cu:75-78).
// The names and argument lists are the reference's (costVolume.cuh:8-14, guidedFilter.cuh:9-39,
// integral.cuh:7, occlusion.cuh:12,19, rgb_to_grayscale.cuh:5,8); the bodies are this repository's own
// sequential restatements of what the DEVICE kernels compute -- in particular guided_filter_onCpu is a
// correct twin (the reference's version writes pixel indices as labels and divides in double,
// SURVEY.md section 4), so that check_errors() can hold it against the GPU result bit for bit.
// Everything is plain f32 arithmetic in source order; build with -ffp-contract=off.
#include <climits>
#include <limits>
#include <vector>

#include "adcensus.cuh"
#include "colourGuidedFilter.cuh"
#include "costVolume.cuh"
#include "crossAggregation.cuh"
#include "crossScale.cuh"
#include "../csrc/smx_cscale_host.h"      // the library's own host arithmetic of the levels: no HIP in it
#include "discontinuityAdjustment.cuh"
#include "filter.cuh"
#include "guidedFilter.cuh"
#include "integral.cuh"
#include "mutualInformation.cuh"
#include "occlusion.cuh"
#include "patchMatch.cuh"
#include "permeability.cuh"
#include "../csrc/smx_perm_host.h"        // the library's own weight table: no HIP in it
#include "regionVoting.cuh"
#include "rgb_to_grayscale.cuh"
#include "scanlineOptimization.cuh"
#include "beliefPropagation.cuh"
#include "sgm.cuh"
#include "speckle.cuh"
#include "uniqueness.cuh"
#include "wmf.cuh"

using std::vector;

// ---- filter.cuh:6 (see the note there: a correct twin of the device path's mean, not the reference's broken body) --------
void boxFilterOnCPU(unsigned char* image, unsigned char* mean, int width, int height) {
    const int R = smx_config().params.radius, area = (2 * R + 1) * (2 * R + 1);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            float sum = 0.0f;
            for (int ix = -R; ix <= R; ++ix)
                for (int iy = -R; iy <= R; ++iy) {
                    const int xx = x + ix, yy = y + iy;
                    sum += (xx >= 0 && xx < width && yy >= 0 && yy < height) ? (float)image[(size_t)yy * width + xx] : 0.0f;
                }
            mean[(size_t)y * width + x] = (unsigned char)(int)(sum / area);
        }
}

// ---- rgb_to_grayscale.cuh ------------------------------------------------------------------
void sumArraysOnHost(unsigned char* image, unsigned char* gray, const int N, int channels) {
    const smx_params& P = smx_config().params;
    for (int k = 0; k < N; ++k) {
        const unsigned char* px = image + (size_t)channels * k;
        const double v = P.r_w * px[0] + P.g_w * px[1] + P.b_w * px[2];
        gray[k] = (unsigned char)v;
    }
}

bool check_errors_grayscale(unsigned char* host, unsigned char* gpu, int len) {
    return check_errors(host, gpu, len);
}

// ---- costVolume.cuh ------------------------------------------------------------------------
int iDivUp(int a, int b) { return (a + b - 1) / b; }

float x_derivativeCPU(unsigned char* im, int col_index, int index, int width) {
    int right, left;
    if (col_index - 1 >= 0 && col_index + 1 < width) { right = im[index + 1]; left = im[index - 1]; }
    else if (col_index + 1 >= width)                 { right = im[index];     left = im[index - 1]; }
    else                                             { right = im[index + 1]; left = im[index];     }
    return 1.0f * (float)(left - right) / 2;
}

void x_derivativeOnCpu(unsigned char* in, float* out, int w, int h) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) out[(size_t)y * w + x] = x_derivativeCPU(in, x, y * w + x, w);
}

void compute_costVolumeOnCpu(unsigned char* i1, unsigned char* i2, float* cost, float* derivative1,
                             float* derivative2, int w1, int w2, int h1, int h2, int size_d, int dmin) {
    (void)h2;
    const smx_params& P = smx_config().params;
    const float alpha = 1.0f * P.alpha, th_color = 1.0f * P.th_color, th_grad = 1.0f * P.th_grad;
    const float border = (1 - alpha) * th_color + 1.0f * alpha * th_grad;
    const size_t n = (size_t)w1 * h1;
    for (int z = 0; z < size_d; ++z) {
        const int d = dmin + z;
        for (int y = 0; y < h1; ++y)
            for (int x = 0; x < w1; ++x) {
                const size_t a = (size_t)y * w1 + x;
                float c = border;
                if (x + d < w2 && x + d >= 0) {
                    const size_t b = a + d;
                    const int di = (int)i1[a] - (int)i2[b];
                    const float t1 = 1.0f * (float)(di < 0 ? -di : di);
                    const float t2 = 1.0f * fabsf(derivative1[a] - derivative2[b]);
                    const float m1 = t1 < th_color ? t1 : th_color;
                    const float m2 = t2 < th_grad ? t2 : th_grad;
                    const float p1 = (1.0f - alpha) * m1;
                    const float p2 = alpha * m2;
                    c = p1 + p2;
                }
                cost[(size_t)z * n + a] = c;
            }
    }
}

void costVolumeOnCPU(unsigned char* i1, unsigned char* i2, float* cost, int w1, int w2, int h1, int h2,
                     int size_d, int dmin) {
    vector<float> g1((size_t)w1 * h1), g2((size_t)w2 * h2);
    x_derivativeOnCpu(i1, g1.data(), w1, h1);
    x_derivativeOnCpu(i2, g2.data(), w2, h2);
    compute_costVolumeOnCpu(i1, i2, cost, g1.data(), g2.data(), w1, w2, h1, h2, size_d, dmin);
}

// ---- integral.cuh --------------------------------------------------------------------------
void integralOnCPU(float* in, float* out, const int w, const int h) {
    for (int y = 0; y < h; ++y) {
        float acc = in[(size_t)y * w];
        out[(size_t)y * w] = acc;
        for (int x = 1; x < w; ++x) {
            acc = in[(size_t)y * w + x] + acc;
            out[(size_t)y * w + x] = acc;
        }
    }
    for (int y = 1; y < h; ++y)
        for (int x = 0; x < w; ++x) out[(size_t)y * w + x] = out[(size_t)y * w + x] + out[(size_t)(y - 1) * w + x];
}

// ---- guidedFilter.cuh ----------------------------------------------------------------------
float computeMeanOnCPU(float* I, float* S, int idx, int idy, const int w, const int h) {
    (void)I;
    const int R = smx_config().params.radius;
    const int y0 = std::max(-1, idy - R - 1), y1 = std::min(h - 1, idy + R);
    const int x0 = std::max(-1, idx - R - 1), x1 = std::min(w - 1, idx + R);
    float val = S[(size_t)y1 * w + x1];
    if (x0 >= 0) val -= S[(size_t)y1 * w + x0];
    if (y0 >= 0) val -= S[(size_t)y0 * w + x1];
    if (x0 >= 0 && y0 >= 0) val += S[(size_t)y0 * w + x0];
    return 1.0f * val / (float)((x1 - x0) * (y1 - y0));
}

void computeBoxFilterOnCPU(float* image, float* integral, float* mean, const int w, const int h) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) mean[(size_t)y * w + x] = computeMeanOnCPU(image, integral, x, y, w, h);
}

void chToFlOnCPU(unsigned char* image, float* result, int len) {
    for (int k = 0; k < len; ++k) result[k] = 1.0f * (float)(int)image[k];
}
void flToChOnCPU(float* image, unsigned char* result, int len) {
    for (int k = 0; k < len; ++k) {
        const int c = (int)image[k];
        result[k] = c > 255 ? 255 : (unsigned char)c;
    }
}
void pixelMultOnCPU(float* a, float* b, float* r, int len) { for (int k = 0; k < len; ++k) r[k] = a[k] * b[k]; }
void pixelSousOnCPU(float* a, float* b, float* r, int len) { for (int k = 0; k < len; ++k) r[k] = a[k] - b[k]; }
void pixelAddOnCPU(float* a, float* b, float* r, int len) { for (int k = 0; k < len; ++k) r[k] = a[k] + b[k]; }
void pixelDivOnCPU(float* a, float* b, float* r, int len) { for (int k = 0; k < len; ++k) r[k] = a[k] / b[k]; }

void dispSelectOnCPU(float* q, float* filter_cost, float* dmap, const int n, int label) {
    for (int k = 0; k < n; ++k)
        if (1.0f * filter_cost[k] >= 1.0f * q[k]) { dmap[k] = (float)label; filter_cost[k] = q[k]; }
}

// What compute_guided_filter computes on the device (guidedFilter.cu:58-238), sequentially.
void guided_filter_onCpu(unsigned char* im1, float* cost, float* filtered_cost, float* dmap,
                         unsigned char* mean, const int w, const int h, const int size_d, int dmin) {
    const int n = w * h;
    const double eps = smx_config().params.eps;
    vector<float> im(n), S(n), mI(n), var(n), t(n), mp(n), mIp(n), a(n), b(n), q(n);
    chToFlOnCPU(im1, im.data(), n);
    integralOnCPU(im.data(), S.data(), w, h);
    computeBoxFilterOnCPU(im.data(), S.data(), mI.data(), w, h);
    if (mean) flToChOnCPU(mI.data(), mean, n);
    pixelMultOnCPU(im.data(), im.data(), t.data(), n);
    integralOnCPU(t.data(), S.data(), w, h);
    computeBoxFilterOnCPU(t.data(), S.data(), var.data(), w, h);
    pixelMultOnCPU(mI.data(), mI.data(), t.data(), n);
    pixelSousOnCPU(var.data(), t.data(), var.data(), n);
    for (int s = 0; s < size_d; ++s) {
        float* p = cost + (size_t)s * n;
        integralOnCPU(p, S.data(), w, h);
        computeBoxFilterOnCPU(p, S.data(), mp.data(), w, h);
        pixelMultOnCPU(im.data(), p, t.data(), n);
        integralOnCPU(t.data(), S.data(), w, h);
        computeBoxFilterOnCPU(t.data(), S.data(), mIp.data(), w, h);
        for (int k = 0; k < n; ++k) {                    // compute_ak_and_bk, guidedFilter.cu:345-354
            const float c = (float)(1.0f / ((double)var[k] + eps));
            const float mm = mI[k] * mp[k];
            a[k] = 1.0f * (mIp[k] - mm) * c;
            const float mb = 1.0f * mI[k] * a[k];
            b[k] = 1.0f * mp[k] - mb;
        }
        integralOnCPU(a.data(), S.data(), w, h);
        computeBoxFilterOnCPU(a.data(), S.data(), t.data(), w, h);      // mean(a)
        integralOnCPU(b.data(), S.data(), w, h);
        computeBoxFilterOnCPU(b.data(), S.data(), mp.data(), w, h);     // mean(b)
        for (int k = 0; k < n; ++k) {                    // compute_q, :363-369
            const float m = t[k] * im[k];
            q[k] = m + mp[k];
        }
        dispSelectOnCPU(q.data(), filtered_cost, dmap, n, dmin + s);
    }
}

// ---- colourGuidedFilter.cuh (not in the reference) ------------------------------------------
// The definition of include/smx.h (above smx_cgf_workspace_bytes), sequentially: integral images as integralOnCPU, box means as
// computeMeanOnCPU with the radius given, the 3 x 3 inverse in double with every product and sum rounded on its own.
namespace {
void cgf_box_mean(const float* img, float* S, float* mean, const int w, const int h, const int R) {
    integralOnCPU(const_cast<float*>(img), S, w, h);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int y0 = std::max(-1, y - R - 1), y1 = std::min(h - 1, y + R);
            const int x0 = std::max(-1, x - R - 1), x1 = std::min(w - 1, x + R);
            float val = S[(size_t)y1 * w + x1];
            if (x0 >= 0) val -= S[(size_t)y1 * w + x0];
            if (y0 >= 0) val -= S[(size_t)y0 * w + x1];
            if (x0 >= 0 && y0 >= 0) val += S[(size_t)y0 * w + x0];
            mean[(size_t)y * w + x] = val / (float)((x1 - x0) * (y1 - y0));
        }
}
}  // namespace

void colour_guided_filterOnCPU(const unsigned char* rgb, int channels, const float* cost, float* filter_cost, float* disp_map,
                               float* agg, const int w, const int h, const int size_d, const int dmin, const int radius,
                               const double eps) {
    const size_t n = (size_t)w * h;
    const int R = std::min(radius, std::max(w, h));      // (a window beyond the image is the image)
    vector<float> I[3], mu[3], inv[6], cov[3], a[4], abar[4];
    vector<float> S(n), t(n), m(n), mp(n), q(n);
    for (int c = 0; c < 3; ++c) {
        I[c].resize(n); mu[c].resize(n); cov[c].resize(n);
        for (size_t k = 0; k < n; ++k) I[c][k] = (float)(int)rgb[k * channels + c];
        cgf_box_mean(I[c].data(), S.data(), mu[c].data(), w, h, R);
    }
    for (int c = 0; c < 4; ++c) { a[c].resize(n); abar[c].resize(n); }
    // v_cc' in the order rr, rg, rb, gg, gb, bb, kept in inv[] until the inverse overwrites them
    static const int pair[6][2] = {{0, 0}, {0, 1}, {0, 2}, {1, 1}, {1, 2}, {2, 2}};
    for (int j = 0; j < 6; ++j) {
        inv[j].resize(n);
        for (size_t k = 0; k < n; ++k) t[k] = I[pair[j][0]][k] * I[pair[j][1]][k];
        cgf_box_mean(t.data(), S.data(), m.data(), w, h, R);
        for (size_t k = 0; k < n; ++k) {
            const float prod = mu[pair[j][0]][k] * mu[pair[j][1]][k];
            inv[j][k] = m[k] - prod;
        }
    }
    for (size_t k = 0; k < n; ++k) {
        const double va = (double)inv[0][k] + eps, vb = (double)inv[1][k], vc = (double)inv[2][k];
        const double vd = (double)inv[3][k] + eps, ve = (double)inv[4][k], vf = (double)inv[5][k] + eps;
        const double A = vd * vf - ve * ve, B = vc * ve - vb * vf, C = vb * ve - vc * vd;
        const double D = va * vf - vc * vc, E = vb * vc - va * ve, F = va * vd - vb * vb;
        const double det = (va * A + vb * B) + vc * C;
        inv[0][k] = (float)(A / det); inv[1][k] = (float)(B / det); inv[2][k] = (float)(C / det);
        inv[3][k] = (float)(D / det); inv[4][k] = (float)(E / det); inv[5][k] = (float)(F / det);
    }
    for (int s = 0; s < size_d; ++s) {
        const float* p = cost + (size_t)s * n;
        cgf_box_mean(p, S.data(), mp.data(), w, h, R);
        for (int c = 0; c < 3; ++c) {
            for (size_t k = 0; k < n; ++k) t[k] = I[c][k] * p[k];
            cgf_box_mean(t.data(), S.data(), m.data(), w, h, R);
            for (size_t k = 0; k < n; ++k) {
                const float prod = mu[c][k] * mp[k];
                cov[c][k] = m[k] - prod;
            }
        }
        for (size_t k = 0; k < n; ++k) {
            const float cr = cov[0][k], cg = cov[1][k], cb = cov[2][k];
            const float r0 = inv[0][k] * cr, r1 = inv[1][k] * cg, r2 = inv[2][k] * cb;
            const float g0 = inv[1][k] * cr, g1 = inv[3][k] * cg, g2 = inv[4][k] * cb;
            const float b0 = inv[2][k] * cr, b1 = inv[4][k] * cg, b2 = inv[5][k] * cb;
            a[0][k] = (r0 + r1) + r2;
            a[1][k] = (g0 + g1) + g2;
            a[2][k] = (b0 + b1) + b2;
            const float s0 = a[0][k] * mu[0][k], s1 = a[1][k] * mu[1][k], s2 = a[2][k] * mu[2][k];
            a[3][k] = mp[k] - ((s0 + s1) + s2);
        }
        for (int c = 0; c < 4; ++c) cgf_box_mean(a[c].data(), S.data(), abar[c].data(), w, h, R);
        for (size_t k = 0; k < n; ++k) {
            const float q0 = abar[0][k] * I[0][k], q1 = abar[1][k] * I[1][k], q2 = abar[2][k] * I[2][k];
            q[k] = ((q0 + q1) + q2) + abar[3][k];
        }
        if (agg) std::memcpy(agg + (size_t)s * n, q.data(), n * sizeof(float));
        dispSelectOnCPU(q.data(), filter_cost, disp_map, (int)n, dmin + s);
    }
}

// ---- crossAggregation.cuh (not in the reference) ------------------------------------------------
// The definition of include/smx.h (above smx_cross_workspace_bytes) in scalar integer arithmetic: every arm walked step by
// step, every sum taken pixel by pixel over the arm.
namespace {
int cross_dist(const unsigned char* a, const unsigned char* b, const int nc) {
    int d = 0;
    for (int c = 0; c < nc; ++c) d = std::max(d, std::abs((int)a[c] - (int)b[c]));
    return d;
}
// the arm of pixel (x, y) in direction (dx, dy)
int cross_arm(const unsigned char* g, const int ch, const int nc, const int w, const int h, const int x, const int y,
              const int dx, const int dy, const smx_cross_params& p) {
    const unsigned char* pp = g + ((size_t)y * w + x) * ch;
    const unsigned char* prev = pp;
    int k = 0;
    for (int j = 1; j <= p.l1; ++j) {
        const int qx = x + j * dx, qy = y + j * dy;
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) break;
        const unsigned char* q = g + ((size_t)qy * w + qx) * ch;
        const int dp = cross_dist(q, pp, nc);
        if (!(dp < p.tau1 && cross_dist(q, prev, nc) < p.tau1 && (j <= p.l2 || dp < p.tau2))) break;
        k = j;
        prev = q;
    }
    return k;
}
// out = the sums of in over the horizontal (vertical == false) or vertical arm of every pixel
void cross_pass(const vector<uint32_t>& in, vector<uint32_t>& out, const vector<int>* arm, const int w, const int h,
                const bool vertical) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            uint32_t s = 0;
            if (vertical) for (int yy = y - arm[2][id]; yy <= y + arm[3][id]; ++yy) s += in[(size_t)yy * w + x];
            else for (int xx = x - arm[0][id]; xx <= x + arm[1][id]; ++xx) s += in[(size_t)y * w + xx];
            out[id] = s;
        }
}
}  // namespace

void cross_aggregateOnCPU(const unsigned char* guide, int channels, const float* cost, float* filter_cost, float* disp_map,
                          float* agg, const int w, const int h, const int size_d, const int dmin, const smx_cross_params& p) {
    const size_t n = (size_t)w * h;
    const int nc = channels == 1 ? 1 : 3;
    static const int dir[4][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}};       // left, right, up, down
    vector<int> arm[4];
    for (int e = 0; e < 4; ++e) {
        arm[e].resize(n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) arm[e][(size_t)y * w + x] = cross_arm(guide, channels, nc, w, h, x, y, dir[e][0], dir[e][1], p);
    }
    // the areas of the two orders: the same sums of 1
    vector<uint32_t> one(n, 1u), t(n), area[2], v(n), s(n);
    for (int order = 0; order < 2; ++order) {
        area[order].resize(n);
        cross_pass(one, t, arm, w, h, order == 1);
        cross_pass(t, area[order], arm, w, h, order == 0);
    }
    vector<float> q(n);
    for (int z = 0; z < size_d; ++z) {
        const float* c = cost + (size_t)z * n;
        for (size_t k = 0; k < n; ++k) v[k] = 16u * (c[k] >= 0.0f ? (c[k] <= 255.0f ? (uint32_t)(int)c[k] : 255u) : 0u);
        for (int i = 0; i < p.iterations; ++i) {
            const int order = i & 1;
            cross_pass(v, t, arm, w, h, order == 1);
            cross_pass(t, s, arm, w, h, order == 0);
            for (size_t k = 0; k < n; ++k) v[k] = (2u * s[k] + area[order][k]) / (2u * area[order][k]);
        }
        for (size_t k = 0; k < n; ++k) q[k] = (float)v[k] * 0.0625f;
        if (agg) std::memcpy(agg + (size_t)z * n, q.data(), n * sizeof(float));
        dispSelectOnCPU(q.data(), filter_cost, disp_map, (int)n, dmin + z);
    }
}

// ---- regionVoting.cuh (not in the reference) -----------------------------------------------------
// The definition of include/smx.h (above smx_vote_workspace_bytes) pixel by pixel: per outlier one histogram over its region,
// walked row by row and pixel by pixel; per remaining outlier the 16 directions one after the other.
void region_voteOnCPU(const unsigned char* guide, int channels, const float* disparity, const float* disparity_right, float* out,
                      const int w, const int h, const int dmin, const int size_d, const smx_vote_params& p,
                      const smx_cross_params& arms) {
    const size_t n = (size_t)w * h;
    const int nc = channels == 1 ? 1 : 3;
    const float vmin = (float)dmin, d_lr = (float)smx_config().params.d_lr;
    static const int dir[4][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}};       // left, right, up, down
    vector<int> arm[4];
    for (int e = 0; e < 4; ++e) {
        arm[e].resize(n);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) arm[e][(size_t)y * w + x] = cross_arm(guide, channels, nc, w, h, x, y, dir[e][0], dir[e][1], arms);
    }
    auto trunc_sat = [](float v) { return v >= 2147483648.0f ? INT_MAX : v < -2147483648.0f ? INT_MIN : (int)v; };
    auto valid = [&](float v) { return std::fabs(v) <= 3.402823466e38f && (float)trunc_sat(v) >= vmin; };
    auto bin = [&](float v) -> int {            // of a voter, else -1
        if (!valid(v)) return -1;
        const long long b = (long long)trunc_sat(v) - dmin;
        return b >= 0 && b < size_d ? (int)b : -1;
    };
    vector<float> cur(disparity, disparity + n), next(n);
    vector<int> hist(size_d, 0);
    for (int k = 0; k < p.iterations; ++k) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t id = (size_t)y * w + x;
                next[id] = cur[id];
                if (valid(cur[id])) continue;
                long long total = 0;
                for (int yy = y - arm[2][id]; yy <= y + arm[3][id]; ++yy) {
                    const size_t c = (size_t)yy * w + x;
                    for (int xx = x - arm[0][c]; xx <= x + arm[1][c]; ++xx) {
                        const int b = bin(cur[(size_t)yy * w + xx]);
                        if (b >= 0) { ++hist[b]; ++total; }
                    }
                }
                int top = 0;
                for (int b = 0; b < size_d; ++b)
                    if (hist[b] >= hist[top]) top = b;         // the largest bin among the largest counts
                if (total > p.tau_s && 100ll * hist[top] > (long long)p.tau_h_pct * total) next[id] = (float)(int)((long long)dmin + top);
                std::fill(hist.begin(), hist.end(), 0);
            }
        cur.swap(next);
    }
    static const int step[16][2] = {{1, 0},  {2, 1},   {1, 1},   {1, 2},   {0, 1},  {-1, 2}, {-1, 1}, {-2, 1},
                                    {-1, 0}, {-2, -1}, {-1, -1}, {-1, -2}, {0, -1}, {1, -2}, {1, -1}, {2, -1}};     // (dx, dy)
    for (size_t id = 0; id < n; ++id) out[id] = cur[id];
    if (!p.interpolate) return;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            if (valid(cur[id])) continue;
            bool mismatch = false;
            if (disparity_right)
                for (int s = 0; s < size_d && !mismatch; ++s) {
                    const long long d = (long long)dmin + s, xr = x + d;
                    if (xr < 0 || xr >= w) continue;
                    volatile float sum = (float)(int)d + disparity_right[(size_t)y * w + (size_t)xr];      // one rounded f32 sum
                    mismatch = std::fabs(sum) <= d_lr;
                }
            bool has = false;
            float best_v = 0.0f;
            int best_d = 0;
            for (int e = 0; e < 16; ++e)
                for (int qx = x + step[e][0], qy = y + step[e][1]; qx >= 0 && qx < w && qy >= 0 && qy < h;
                     qx += step[e][0], qy += step[e][1]) {
                    const size_t q = (size_t)qy * w + qx;
                    if (bin(cur[q]) < 0) continue;
                    const int dist = cross_dist(guide + q * channels, guide + id * channels, nc);
                    // strict comparisons: the first in the order among equals
                    if (!has || (mismatch ? dist < best_d : cur[q] > best_v)) out[id] = cur[q];
                    if (!has || dist < best_d) best_d = dist;
                    if (!has || cur[q] > best_v) best_v = cur[q];
                    has = true;
                    break;
                }
        }
}

// ---- discontinuityAdjustment.cuh (not in the reference) ------------------------------------------
// The definition of include/smx.h (above smx_adjust_workspace_bytes) pixel by pixel: per round a snapshot, per labelled pixel its
// up to four candidates in the order left, right, up, down.  The sub-pixel formula is smx_subpixel_delta's, restated.
static float subpixel_deltaOnCPU(int mode, float c0, float lo, float hi) {
    if (lo != lo || hi != hi) return 0.0f;
    const float a = lo - c0, b = hi - c0;
    const float den = mode == SMX_SUBPIX_PARABOLA ? a + b : fmaxf(a, b);
    const float d = (a - b) / (2.0f * den);
    return d - d == 0.0f ? d : 0.0f;
}

void discontinuityAdjustOnCPU(const float* disparity, const float* agg, float* out, const int w, const int h, const int dmin,
                              const int size_d, const smx_adjust_params& p, int subpix_mode, float* sub) {
    const size_t n = (size_t)w * h;
    auto slice = [&](float v) -> int {          // of a labelled value, else -1
        if (!(std::fabs(v) < 1099511627776.0f) || v != std::trunc(v)) return -1;
        const long long z = (long long)v - dmin;
        return z >= 0 && z < size_d ? (int)z : -1;
    };
    static const int step[4][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}};      // (dx, dy): left, right, up, down
    vector<float> cur(disparity, disparity + n), next(n);
    for (int k = 0; k < p.iterations; ++k) {
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t id = (size_t)y * w + x;
                next[id] = cur[id];
                const int z = slice(cur[id]);
                if (z < 0) continue;
                float best = agg[(size_t)z * n + id];
                int zb = z;
                for (int e = 0; e < (p.vertical ? 4 : 2); ++e) {
                    const int qx = x + step[e][0], qy = y + step[e][1];
                    if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                    const size_t q = (size_t)qy * w + qx;
                    const int zq = slice(cur[q]);
                    if (zq < 0 || std::abs(zq - z) < p.tau_e) continue;
                    const float c = agg[(size_t)zq * n + id];
                    if (c < best) { best = c; zb = zq; next[id] = cur[q]; }
                }
                if (zb != z && sub) {
                    const float nan = std::numeric_limits<float>::quiet_NaN();
                    const float lo = zb > 0 ? agg[(size_t)(zb - 1) * n + id] : nan;
                    const float hi = zb + 1 < size_d ? agg[(size_t)(zb + 1) * n + id] : nan;
                    sub[id] = next[id] + subpixel_deltaOnCPU(subpix_mode, best, lo, hi);
                }
            }
        cur.swap(next);
    }
    for (size_t id = 0; id < n; ++id) out[id] = cur[id];
}

// ---- crossScale.cuh (not in the reference) ---------------------------------------------------------
// The definition of include/smx.h (above smx_cscale_params), scalar: the pyramid on integers, the combination as one f32 product
// per level and f32 sums in the order of the levels, the winner by `best >= q` over ascending slices.
void pyrDownOnCPU(const unsigned char* src, unsigned char* dst, const int w, const int h, const int channels) {
    static const int tap[5] = {1, 4, 6, 4, 1};
    auto at = [](int i, int n) {            // reflect-101, then clamped (n of 1 or 2)
        i = i < 0 ? -i : i;
        i = i >= n ? 2 * (n - 1) - i : i;
        return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
    };
    const int wo = (w + 1) / 2, ho = (h + 1) / 2;
    for (int yo = 0; yo < ho; ++yo)
        for (int xo = 0; xo < wo; ++xo)
            for (int c = 0; c < channels; ++c) {
                int t = 0;
                for (int j = 0; j < 5; ++j) {
                    const size_t row = (size_t)at(2 * yo - 2 + j, h) * w;
                    int r = 0;
                    for (int i = 0; i < 5; ++i) r += tap[i] * (int)src[(row + at(2 * xo - 2 + i, w)) * channels + c];
                    t += tap[j] * r;
                }
                dst[((size_t)yo * wo + xo) * channels + c] = (unsigned char)((t + 128) >> 8);
            }
}

void crossScaleOnCPU(const float* const* levels, float* out, float* best, float* disp_map, const int w, const int h, const int dmin,
                     const int size_d, const smx_cscale_params& p) {
    float wt[SMX_CSCALE_MAX_SCALES];
    if (!smx::cscale_params_ok(&p)) return;
    smx::cscale_weights(&p, wt);        // (what smx_cscale_weights and smx_cscale_level run)
    int ws[SMX_CSCALE_MAX_SCALES], hs[SMX_CSCALE_MAX_SCALES], lo[SMX_CSCALE_MAX_SCALES], ds[SMX_CSCALE_MAX_SCALES];
    for (int s = 0; s < p.scales; ++s) smx::cscale_level(w, h, dmin, size_d, s, &ws[s], &hs[s], &lo[s], &ds[s]);
    const size_t n = (size_t)w * h;
    const uint32_t none = 0x7FFFFFFFu;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            float m = std::numeric_limits<float>::infinity();
            int zm = -1;
            for (int z = 0; z < size_d; ++z) {
                float o = wt[0] * levels[0][(size_t)z * n + id];
                for (int s = 1; s < p.scales; ++s) {
                    const size_t cell = ((size_t)(((dmin + z) >> s) - lo[s]) * hs[s] + (size_t)(y >> s)) * ws[s] + (size_t)(x >> s);
                    const float t = wt[s] * levels[s][cell];
                    o = o + t;
                }
                out[(size_t)z * n + id] = o;
                if (o <= m) { m = o; zm = z; }
            }
            if (best) {
                if (zm < 0) memcpy(&best[id], &none, 4);
                else best[id] = m == 0.0f ? 0.0f : m;
            }
            if (disp_map) disp_map[id] = (float)(dmin + (zm < 0 ? 0 : zm));
        }
}

// ---- patchMatch.cuh (not in the reference) ---------------------------------------------------------
// The definition of include/smx.h (above smx_pm_params), scalar and sequential: a pixel of one colour reads pixels of the other
// colour only, so a pass may run in place.
namespace {

uint32_t pm_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
float pm_uniform(uint32_t seed, uint32_t view, uint32_t pix, uint32_t draw) {
    const uint32_t h = pm_fmix32(pm_fmix32(pm_fmix32(seed + 0x9E3779B9u * (view + 1u)) ^ pix) ^ draw);
    return (float)(h >> 8) * 5.9604644775390625e-08f;
}
float pm_clamp(float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; }

struct PmView {
    const unsigned char* own;
    vector<float> g, io, go;       // the own gradient; gray and gradient of the other view as f32
    int w, h, r, size_d, view;
    float dmin, dmax, alpha, oma, th_color, th_grad, border;
    const float* tab;
    float *a, *b, *d0, *m;         // the state [h][w] each
};

vector<float> pm_xgrad(const unsigned char* img, int w, int h) {
    vector<float> g((size_t)w * h, 0.0f);
    if (w < 2) return g;
    for (int y = 0; y < h; ++y) {
        const unsigned char* r = img + (size_t)y * w;
        for (int x = 0; x < w; ++x) {
            const int c1 = x + 1 < w ? r[x + 1] : r[x], c2 = x - 1 >= 0 ? r[x - 1] : r[x];
            g[(size_t)y * w + x] = 1.0f * (float)(c2 - c1) / 2;
        }
    }
    return g;
}

float pm_plane_cost(const PmView& v, int x, int y, float a, float b, float d0) {
    const int w = v.w, h = v.h, r = v.r;
    const int ip = v.own[(size_t)y * w + x];
    float acc = 0.0f;
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= h) continue;
        const size_t row = (size_t)qy * w;
        const float bdy = b * (float)dy;
        for (int dx = -r; dx <= r; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= w) continue;
            const int iq = v.own[row + qx];
            const float wgt = v.tab[std::abs(ip - iq)];
            const float d = (d0 + a * (float)dx) + bdy;
            const float xs = (float)qx + d;
            float rho = v.border;
            if (d >= v.dmin && d <= v.dmax && xs >= 0.0f && xs <= (float)(w - 1)) {
                const float fl = std::floor(xs);
                const int i = (int)fl, i1 = i + 1 < w ? i + 1 : w - 1;
                const float t = xs - fl;
                const float ii = v.io[row + i] + t * (v.io[row + i1] - v.io[row + i]);
                const float gi = v.go[row + i] + t * (v.go[row + i1] - v.go[row + i]);
                const float t1 = std::fabs((float)iq - ii), t2 = std::fabs(v.g[row + qx] - gi);
                const float m1 = t1 < v.th_color ? t1 : v.th_color, m2 = t2 < v.th_grad ? t2 : v.th_grad;
                const float ca = v.oma * m1, cb = v.alpha * m2;
                rho = ca + cb;
            }
            const float term = wgt * rho;
            acc = acc + term;
        }
    }
    return acc;
}

PmView pm_view(const unsigned char* own, const unsigned char* other, int view, int w, int h, int size_d, int dmin,
               const smx_pm_params& p, const float* tab, float* planes, float* cost) {
    const smx_params& P = smx_config().params;
    const size_t n = (size_t)w * h;
    PmView v;
    v.own = own;
    v.g = pm_xgrad(own, w, h);
    v.go = pm_xgrad(other, w, h);
    v.io.assign(other, other + n);
    v.w = w; v.h = h; v.r = p.radius; v.size_d = size_d; v.view = view;
    v.dmin = (float)dmin; v.dmax = (float)(dmin + size_d - 1);
    v.alpha = 1.0f * P.alpha; v.oma = 1.0f - v.alpha;
    v.th_color = 1.0f * P.th_color; v.th_grad = 1.0f * P.th_grad;
    const float ca = v.oma * v.th_color, cb = 1.0f * v.alpha * v.th_grad;
    v.border = ca + cb;
    v.tab = tab;
    v.a = planes; v.b = planes + n; v.d0 = planes + 2 * n; v.m = cost;
    return v;
}

void pm_try(const PmView& v, size_t id, int x, int y, float a, float b, float d0) {
    const float c = pm_plane_cost(v, x, y, a, b, d0);
    if (c < v.m[id]) { v.a[id] = a; v.b[id] = b; v.d0[id] = d0; v.m[id] = c; }
}

void pm_pass(const PmView& v, const smx_pm_params& p, int it, int colour) {
    static const int nb[8][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}, {-5, 0}, {5, 0}, {0, -5}, {0, 5}};      // (dx, dy)
    const int w = v.w, h = v.h;
    const float ms = (float)p.max_slope;
    for (int y = 0; y < h; ++y)
        for (int x = (y + colour) & 1; x < w; x += 2) {
            const size_t id = (size_t)y * w + x;
            for (const auto& e : nb) {
                const int nx = x + e[0], ny = y + e[1];
                if (nx < 0 || nx >= w || ny < 0 || ny >= h) continue;
                const size_t q = (size_t)ny * w + nx;
                const float d = (v.d0[q] + v.a[q] * (float)(x - nx)) + v.b[q] * (float)(y - ny);
                if (d >= v.dmin && d <= v.dmax) pm_try(v, id, x, y, v.a[q], v.b[q], d);
            }
            float dd = (float)(v.size_d - 1) * 0.5f, ds = ms * 0.5f;
            for (int k = 0; dd >= 0.1f; ++k) {
                const uint32_t base = 3u + 3u * (uint32_t)(it * 32 + k);
                const float r0 = 2.0f * pm_uniform(p.seed, v.view, (uint32_t)id, base) - 1.0f;
                const float r1 = 2.0f * pm_uniform(p.seed, v.view, (uint32_t)id, base + 1u) - 1.0f;
                const float r2 = 2.0f * pm_uniform(p.seed, v.view, (uint32_t)id, base + 2u) - 1.0f;
                pm_try(v, id, x, y, pm_clamp(v.a[id] + r1 * ds, -ms, ms), pm_clamp(v.b[id] + r2 * ds, -ms, ms),
                       pm_clamp(v.d0[id] + r0 * dd, v.dmin, v.dmax));
                dd = dd * 0.5f;
                ds = ds * 0.5f;
            }
        }
}

void pm_view_propagation(const PmView& v, const vector<float>& other) {      // other: the other view's planes [3][h][w], a snapshot
    const int w = v.w, h = v.h;
    const size_t n = (size_t)w * h;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            int xo = (int)std::floor(((float)x + v.d0[id]) + 0.5f);
            xo = xo < 0 ? 0 : xo > w - 1 ? w - 1 : xo;
            const size_t q = (size_t)y * w + xo;
            const float d = -other[2 * n + q];
            if (d >= v.dmin && d <= v.dmax) pm_try(v, id, x, y, -other[q], -other[n + q], d);
        }
}

vector<float> pm_table(const smx_pm_params& p) {
    vector<float> tab(256);
    for (int k = 0; k < 256; ++k) tab[k] = (float)std::exp(-(double)k / p.gamma);
    return tab;
}

}  // namespace

void pmPlaneCostOnCPU(const unsigned char* left, const unsigned char* right, const float* planes, float* cost, const int w,
                      const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p) {
    const size_t n = (size_t)w * h;
    const vector<float> tab = pm_table(p);
    for (int view = 0; view < 2; ++view) {
        const PmView v = pm_view(view ? right : left, view ? left : right, view, w, h, size_d, view ? dminr : dminl, p, tab.data(),
                                 const_cast<float*>(planes) + 3 * n * view, cost + n * view);
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t id = (size_t)y * w + x;
                v.m[id] = pm_plane_cost(v, x, y, v.a[id], v.b[id], v.d0[id]);
            }
    }
}

void patchMatchOnCPU(const unsigned char* left, const unsigned char* right, float* planes, float* cost, float* disp, float* label,
                     const int w, const int h, const int size_d, const int dminl, const int dminr, const smx_pm_params& p) {
    const size_t n = (size_t)w * h;
    const vector<float> tab = pm_table(p);
    const float ms = (float)p.max_slope;
    PmView views[2] = {pm_view(left, right, 0, w, h, size_d, dminl, p, tab.data(), planes, cost),
                       pm_view(right, left, 1, w, h, size_d, dminr, p, tab.data(), planes + 3 * n, cost + n)};
    for (const PmView& v : views)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t id = (size_t)y * w + x;
                v.d0[id] = v.dmin + pm_uniform(p.seed, v.view, (uint32_t)id, 0) * (float)(size_d - 1);
                v.a[id] = (2.0f * pm_uniform(p.seed, v.view, (uint32_t)id, 1) - 1.0f) * ms;
                v.b[id] = (2.0f * pm_uniform(p.seed, v.view, (uint32_t)id, 2) - 1.0f) * ms;
                v.m[id] = pm_plane_cost(v, x, y, v.a[id], v.b[id], v.d0[id]);
            }
    for (int it = 0; it < p.iterations; ++it) {
        for (const PmView& v : views) {
            pm_pass(v, p, it, it & 1);
            pm_pass(v, p, it, (it & 1) ^ 1);
        }
        const vector<float> snap_l(planes, planes + 3 * n), snap_r(planes + 3 * n, planes + 6 * n);
        pm_view_propagation(views[0], snap_r);
        pm_view_propagation(views[1], snap_l);
    }
    for (const PmView& v : views)
        for (size_t id = 0; id < n; ++id) {
            disp[n * v.view + id] = v.d0[id];
            label[n * v.view + id] = pm_clamp(std::floor(v.d0[id] + 0.5f), v.dmin, v.dmax);
        }
}

// ---- permeability.cuh (not in the reference) -------------------------------------------------------
// The definition of include/smx.h (above smx_perm_params), scalar: per slice and row LR, RL and Hh, then per column of Hh TB, BT
// and out; every product and sum an f32 of its own (the file is compiled with -ffp-contract=off).  The winner by `best >= q`
// over ascending slices.
void permeabilityOnCPU(const float* volume, const unsigned char* guide, const int channels, float* out, float* best, float* disp_map,
                       const int w, const int h, const int dmin, const int size_d, const smx_perm_params& p) {
    if (!smx::perm_params_ok(&p)) return;
    float t[256];
    smx::perm_table(&p, t);              // (what smx_perm_table runs)
    const size_t n = (size_t)w * h;
    auto diff = [&](size_t a, size_t b) {
        int d = 0;
        for (int c = 0; c < (channels == 1 ? 1 : 3); ++c) {
            const int e = std::abs((int)guide[a * channels + c] - (int)guide[b * channels + c]);
            d = e > d ? e : d;
        }
        return d;
    };
    std::vector<float> mu_h(n, 0.0f), mu_v(n, 0.0f), hh(n), fwd((size_t)(w > h ? w : h)), slice(n);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            if (x >= 1) mu_h[id] = t[diff(id, id - 1)];
            if (y >= 1) mu_v[id] = t[diff(id, id - (size_t)w)];
        }
    std::vector<float> m(n, std::numeric_limits<float>::infinity());
    std::vector<int> zm(n, -1);
    for (int z = 0; z < size_d; ++z) {
        const float* C = volume + (size_t)z * n;
        for (int y = 0; y < h; ++y) {
            const float* c = C + (size_t)y * w;
            const float* mu = mu_h.data() + (size_t)y * w;
            fwd[0] = c[0];
            for (int x = 1; x < w; ++x) {
                const float pr = mu[x] * fwd[(size_t)x - 1];
                fwd[(size_t)x] = c[x] + pr;
            }
            float rl = c[w - 1];
            for (int x = w - 1; x >= 0; --x) {
                if (x < w - 1) {
                    const float pr = mu[x + 1] * rl;
                    rl = c[x] + pr;
                }
                const float s = fwd[(size_t)x] + rl;
                hh[(size_t)y * w + x] = s - c[x];
            }
        }
        for (int x = 0; x < w; ++x) {
            fwd[0] = hh[(size_t)x];
            for (int y = 1; y < h; ++y) {
                const float pr = mu_v[(size_t)y * w + x] * fwd[(size_t)y - 1];
                fwd[(size_t)y] = hh[(size_t)y * w + x] + pr;
            }
            float bt = hh[(size_t)(h - 1) * w + x];
            for (int y = h - 1; y >= 0; --y) {
                const size_t id = (size_t)y * w + x;
                if (y < h - 1) {
                    const float pr = mu_v[id + (size_t)w] * bt;
                    bt = hh[id] + pr;
                }
                const float s = fwd[(size_t)y] + bt;
                slice[id] = s - hh[id];
            }
        }
        for (size_t id = 0; id < n; ++id) {
            const float o = slice[id];
            if (out) out[(size_t)z * n + id] = o;
            if (o <= m[id]) { m[id] = o; zm[id] = z; }
        }
    }
    const uint32_t none = 0x7FFFFFFFu;
    for (size_t id = 0; id < n; ++id) {
        if (best) {
            if (zm[id] < 0) memcpy(&best[id], &none, 4);
            else best[id] = m[id] == 0.0f ? 0.0f : m[id];
        }
        if (disp_map) disp_map[id] = (float)(dmin + (zm[id] < 0 ? 0 : zm[id]));
    }
}

// ---- occlusion.cuh -------------------------------------------------------------------------
void detect_occlusionOnCPU(float* disparityLeft, float* disparityRight, const int dOcclusion, const int w,
                           const int h) {
    const int d_lr = smx_config().params.d_lr;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t id = (size_t)y * w + x;
            const int d = (int)disparityLeft[id];
            if (x + d < 0 || x + d >= w || fabsf((float)d + disparityRight[id + d]) > (float)d_lr)
                disparityLeft[id] = (float)dOcclusion;
        }
}

void fill_occlusionOnCPU(float* disparity, const int w, const int h, const float vMin) {
    vector<float> row(w);
    for (int y = 0; y < h; ++y) {
        float* r = disparity + (size_t)y * w;
        std::copy(r, r + w, row.begin());       // snapshot: every pixel sees the unfilled row
        for (int x = 0; x < w; ++x) {
            if ((float)(int)row[x] >= vMin) continue;
            float left = vMin, right = vMin;
            for (int k = x; k >= 0; --k) if (row[k] >= vMin) { left = row[k]; break; }
            for (int k = x; k < w; ++k) if (row[k] >= vMin) { right = row[k]; break; }
            r[x] = left > right ? left : right;
        }
    }
}

// ---- wmf.cuh (not in the reference) ----------------------------------------------------------
// The weighted median of include/smx.h pixel by pixel: weight tables from the formula in double, one label histogram
// per window, the smallest label whose cumulative weight reaches half the total.
void weighted_medianOnCPU(const unsigned char* guide, const float* disparity, const float* select, float* out,
                          const int w, const int h, int dmin, int size_d, const smx_wmf_params& p) {
    const int R = p.radius;
    vector<uint32_t> ws(2 * R * R + 1), wc(256), hist(size_d, 0);
    for (int k = 0; k <= 2 * R * R; ++k)
        ws[k] = k == 0 ? 1023 : (uint32_t)std::floor(1023.0 * std::exp(-(double)k / (p.sigma_s * p.sigma_s)) + 0.5);
    for (int t = 0; t < 256; ++t)
        wc[t] = t == 0 ? 1023 : (uint32_t)std::floor(1023.0 * std::exp(-(double)t * t / (p.sigma_c * p.sigma_c)) + 0.5);
    auto label = [&](float v) -> int {          // v - dmin for an integer v in range, else -1 (counts for nothing)
        if (!(std::fabs(v) < 2147483648.0f)) return -1;
        const int iv = (int)v;
        if ((float)iv != v) return -1;
        const long long k = (long long)iv - dmin;
        return (k >= 0 && k < size_d) ? (int)k : -1;
    };
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t i = (size_t)y * w + x;
            out[i] = disparity[i];
            if (select) {
                const float s = select[i];
                if (!std::isfinite(s) || !(std::trunc((double)s) < (double)dmin)) continue;
            }
            uint32_t total = 0;
            for (int qy = std::max(0, y - R); qy <= std::min(h - 1, y + R); ++qy)
                for (int qx = std::max(0, x - R); qx <= std::min(w - 1, x + R); ++qx) {
                    const size_t j = (size_t)qy * w + qx;
                    const int k = label(disparity[j]);
                    if (k < 0) continue;
                    const int t = std::abs((int)guide[i] - (int)guide[j]);
                    const uint32_t wt = ws[(qx - x) * (qx - x) + (qy - y) * (qy - y)] * wc[t];
                    hist[k] += wt;
                    total += wt;
                }
            uint32_t cum = 0;
            bool found = false;
            for (int k = 0; k < size_d; ++k) {
                cum += hist[k];
                hist[k] = 0;
                if (!found && total && 2 * cum >= total) { out[i] = (float)(dmin + k); found = true; }
            }
        }
}

// ---- speckle.cuh (not in the reference) ------------------------------------------------------
// The speckle filter of include/smx.h as a flood fill: one breadth-first search per component.
void speckle_filterOnCPU(const float* disparity, float* out, const int w, const int h, float vmin, float new_val,
                         const smx_speckle_params& p) {
    const size_t n = (size_t)w * h;
    auto counts = [&](float v) {
        if (!(std::fabs(v) <= 3.402823466e38f)) return false;
        const float t = v >= 2147483648.0f ? 2147483648.0f : v < -2147483648.0f ? -2147483648.0f : (float)(int)v;
        return t >= vmin;
    };
    vector<char> seen(n, 0);
    vector<size_t> comp;
    for (size_t i = 0; i < n; ++i) out[i] = disparity[i];
    for (size_t s = 0; s < n; ++s) {
        if (seen[s] || !counts(disparity[s])) continue;
        comp.assign(1, s);
        seen[s] = 1;
        for (size_t k = 0; k < comp.size(); ++k) {
            const size_t i = comp[k];
            const int x = (int)(i % w), y = (int)(i / w);
            const size_t nb[4] = {i - 1, i + 1, i - w, i + w};
            const bool in[4] = {x > 0, x + 1 < w, y > 0, y + 1 < h};
            for (int d = 0; d < 4; ++d) {
                if (!in[d] || seen[nb[d]] || !counts(disparity[nb[d]])) continue;
                volatile float diff = disparity[i] - disparity[nb[d]];     // one rounded f32 difference
                if (!(std::fabs(diff) <= p.max_diff)) continue;
                seen[nb[d]] = 1;
                comp.push_back(nb[d]);
            }
        }
        if (comp.size() <= (size_t)p.max_size)
            for (size_t i : comp) out[i] = new_val;
    }
}

// ---- uniqueness.cuh (not in the reference) ---------------------------------------------------
// The uniqueness test of include/smx.h by the definition: the winner first, then a second loop over the slices at least two
// away from it.  (The kernels keep sec in one pass; this is the check of that streaming form.)
void uniqueness_onCPU(const float* agg, const float* disparity, float* out, float* margin, const int w, const int h,
                      const int size_d, float ratio, float vmin, float new_val) {
    const size_t n = (size_t)w * h;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    auto counts = [&](float v) {
        if (!(std::fabs(v) <= 3.402823466e38f)) return false;
        const float t = v >= 2147483648.0f ? 2147483648.0f : v < -2147483648.0f ? -2147483648.0f : (float)(int)v;
        return t >= vmin;
    };
    for (size_t i = 0; i < n; ++i) {
        // smallest cost, the last slice among equal costs, a NaN never
        int zs = -1;
        float c0 = inf;
        for (int z = 0; z < size_d; ++z) {
            const float v = agg[(size_t)z * n + i];
            if (v <= c0) { c0 = v; zs = z; }
        }
        out[i] = disparity[i];
        if (zs < 0) {
            if (margin) margin[i] = nan;
            continue;
        }
        if (c0 == 0.0f) c0 = 0.0f;          // (the key folds -0 to +0)
        float sec = inf;
        for (int z = 0; z < size_d; ++z) {
            const float v = agg[(size_t)z * n + i];
            if ((z <= zs - 2 || z >= zs + 2) && v < sec) sec = v;
        }
        if (!(sec < inf)) {
            if (margin) margin[i] = inf;
            continue;
        }
        volatile float d = sec - c0;         // one rounded f32 difference, one rounded product
        volatile float bound = ratio * std::fabs(c0);
        if (margin) margin[i] = d;
        if (ratio > 0.0f && d < bound && counts(disparity[i])) out[i] = new_val;
    }
}

// ---- adcensus.cuh (not in the reference) -----------------------------------------------------
// The AD-Census cost by the definition in include/smx.h, one cell at a time: the census codes of the two gray images
// (replicate clamp, bit k in window order with the centre skipped), then per cell the truncated Hamming distance, the sum of
// the absolute differences over the channels, two table reads and one f32 addition.
void adcensus_costOnCPU(const unsigned char* i1, const unsigned char* i2, const unsigned char* g1, const unsigned char* g2,
                        int channels, float* cost, const int w, const int h, const int size_d, const int dmin,
                        const smx_adcensus_params& p, const float* table) {
    const size_t n = (size_t)w * h;
    const int rx = p.census.rx, ry = p.census.ry, nbits = (2 * rx + 1) * (2 * ry + 1) - 1;
    const int t = p.census.th < nbits ? p.census.th : nbits, nch = p.colour ? 3 : 1;
    vector<uint64_t> code[2] = {vector<uint64_t>(n), vector<uint64_t>(n)};
    const unsigned char* gray[2] = {g1, g2};
    for (int v = 0; v < 2; ++v)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const unsigned char c = gray[v][(size_t)y * w + x];
                uint64_t bits = 0;
                int k = 0;
                for (int dy = -ry; dy <= ry; ++dy)
                    for (int dx = -rx; dx <= rx; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        const int yy = y + dy < 0 ? 0 : y + dy > h - 1 ? h - 1 : y + dy;
                        const int xx = x + dx < 0 ? 0 : x + dx > w - 1 ? w - 1 : x + dx;
                        if (gray[v][(size_t)yy * w + xx] < c) bits |= (uint64_t)1 << k;
                        ++k;
                    }
                code[v][(size_t)y * w + x] = bits;
            }
    const float border = table[t] + table[64 + 255 * nch];
    for (int z = 0; z < size_d; ++z)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const long long xx = (long long)x + dmin + z;
                float* out = cost + (size_t)z * n + (size_t)y * w + x;
                if (xx < 0 || xx >= w) { *out = border; continue; }
                const size_t a = (size_t)y * w + x, b = (size_t)y * w + (size_t)xx;
                const int pc = __builtin_popcountll(code[0][a] ^ code[1][b]);
                const int hc = pc < t ? pc : t;
                int s = 0;
                for (int c = 0; c < nch; ++c) {
                    const int d = (int)i1[a * channels + c] - (int)i2[b * channels + c];
                    s += d < 0 ? -d : d;
                }
                *out = table[hc] + table[64 + s];
            }
}

// ---- mutualInformation.cuh (not in the reference) ---------------------------------------------
// The joint histogram and the cost by the definition in include/smx.h, one pixel and one cell at a time.
void mi_histogramOnCPU(const unsigned char* left, const unsigned char* right, const float* disp, float mark, unsigned int* hist,
                       const int w, const int h) {
    for (size_t i = 0; i < (size_t)SMX_MI_LEVELS * SMX_MI_LEVELS; ++i) hist[i] = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t a = (size_t)y * w + x;
            if (disp[a] == mark) continue;
            const long long xx = (long long)x + (long long)(int)disp[a];
            if (xx < 0 || xx >= w) continue;
            ++hist[(size_t)left[a] * SMX_MI_LEVELS + right[(size_t)y * w + (size_t)xx]];
        }
}

void mi_costOnCPU(const unsigned char* table, const unsigned char* left, const unsigned char* right, int view, float* cost,
                  const int w, const int h, const int size_d, const int dmin) {
    const size_t n = (size_t)w * h;
    for (int z = 0; z < size_d; ++z)
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                const long long xx = (long long)x + dmin + z;
                float* out = cost + (size_t)z * n + (size_t)y * w + x;
                if (xx < 0 || xx >= w) { *out = 255.0f; continue; }
                const size_t a = (size_t)y * w + x, b = (size_t)y * w + (size_t)xx;
                // the left view reads T[L[a]][R[b]], the right view T[L[b]][R[a]]
                *out = (float)(view ? table[(size_t)left[b] * SMX_MI_LEVELS + right[a]] : table[(size_t)left[a] * SMX_MI_LEVELS + right[b]]);
            }
}

// ---- sgm.cuh (not in the reference) ----------------------------------------------------------
// Semi-global matching by the definition in include/smx.h: per direction one pass over the image in path order, every
// pixel from its predecessor p - r, integers throughout.
void sgm_aggregateOnCPU(const float* cost, float* agg, float* best, float* disp_map, const int w, const int h,
                        const int size_d, const int dmin, const smx_sgm_params& p) {
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    const size_t n = (size_t)w * h;
    vector<int> C(n * size_d), L(n * size_d), S(n * size_d, 0);     // [pixel][d]
    for (int d = 0; d < size_d; ++d)
        for (size_t i = 0; i < n; ++i) {
            const float c = cost[(size_t)d * n + i];
            C[i * size_d + d] = c >= 0.0f ? (c <= 255.0f ? (int)c : 255) : 0;
        }
    for (int r = 0; r < p.paths; ++r) {
        const int dx = dirs[r][0], dy = dirs[r][1];
        for (int iy = 0; iy < h; ++iy) {
            const int y = dy >= 0 ? iy : h - 1 - iy;
            for (int ix = 0; ix < w; ++ix) {
                const int x = dx >= 0 ? ix : w - 1 - ix;
                const int px = x - dx, py = y - dy;
                int* cur = &L[((size_t)y * w + x) * size_d];
                const int* c = &C[((size_t)y * w + x) * size_d];
                if (px < 0 || px >= w || py < 0 || py >= h) {
                    for (int d = 0; d < size_d; ++d) cur[d] = c[d];
                } else {
                    const int* prev = &L[((size_t)py * w + px) * size_d];
                    int m = prev[0];
                    for (int d = 1; d < size_d; ++d) m = prev[d] < m ? prev[d] : m;
                    for (int d = 0; d < size_d; ++d) {
                        int t = prev[d] < m + p.p2 ? prev[d] : m + p.p2;
                        if (d - 1 >= 0 && prev[d - 1] + p.p1 < t) t = prev[d - 1] + p.p1;
                        if (d + 1 < size_d && prev[d + 1] + p.p1 < t) t = prev[d + 1] + p.p1;
                        cur[d] = c[d] + t - m;
                    }
                }
                int* s = &S[((size_t)y * w + x) * size_d];
                for (int d = 0; d < size_d; ++d) s[d] += cur[d];
            }
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const int* s = &S[i * size_d];
        int z = 0;
        for (int d = 1; d < size_d; ++d)
            if (s[d] <= s[z]) z = d;                 // the last slice of equal sums wins
        if (best) best[i] = (float)s[z];
        if (disp_map) disp_map[i] = (float)(dmin + z);
        if (agg)
            for (int d = 0; d < size_d; ++d) agg[(size_t)d * n + i] = (float)s[d];
    }
}

// ---- beliefPropagation.cuh (not in the reference) --------------------------------------------
// Hierarchical belief propagation by the definition in include/smx.h: the pyramid of data terms, then level by level the
// checkerboard iterations, every message from the sender's data term and its other three messages through the two-pass
// distance transform; integers throughout.  Messages: [level][slot][pixel][z], slot 0 from the left, 1 right, 2 upper, 3 lower.
void beliefPropagationOnCPU(const float* cost, float* agg, float* best, float* disp_map, const int w, const int h,
                            const int size_d, const int dmin, const smx_bp_params& p) {
    const size_t n = (size_t)w * h;
    const int D = size_d;
    vector<int> lw(p.levels), lh(p.levels);
    vector<vector<int>> data(p.levels);
    lw[0] = w; lh[0] = h;
    for (int l = 1; l < p.levels; ++l) { lw[l] = (lw[l - 1] + 1) / 2; lh[l] = (lh[l - 1] + 1) / 2; }
    data[0].resize(n * D);
    for (int d = 0; d < D; ++d)
        for (size_t i = 0; i < n; ++i) {
            const float t = cost[(size_t)d * n + i] * p.data_scale;
            data[0][i * D + d] = t >= 0.0f ? (t <= 255.0f ? (int)t : 255) : 0;
        }
    for (int l = 1; l < p.levels; ++l) {
        data[l].assign((size_t)lw[l] * lh[l] * D, 0);
        for (int y = 0; y < lh[l - 1]; ++y)
            for (int x = 0; x < lw[l - 1]; ++x) {
                const int* src = &data[l - 1][((size_t)y * lw[l - 1] + x) * D];
                int* dst = &data[l][((size_t)(y / 2) * lw[l] + x / 2) * D];
                for (int d = 0; d < D; ++d) dst[d] += src[d];
            }
    }
    static const int from[4][2] = {{-1, 0}, {1, 0}, {0, -1}, {0, 1}};
    vector<int> msg, coarse, out(D);
    for (int l = p.levels - 1; l >= 0; --l) {
        const int cw = lw[l], ch = lh[l];
        const size_t cells = (size_t)cw * ch;
        msg.assign(4 * cells * D, 0);
        if (l < p.levels - 1) {
            const size_t pcells = (size_t)lw[l + 1] * lh[l + 1];
            for (int k = 0; k < 4; ++k)
                for (int y = 0; y < ch; ++y)
                    for (int x = 0; x < cw; ++x)
                        for (int d = 0; d < D; ++d)
                            msg[(k * cells + (size_t)y * cw + x) * D + d] =
                                coarse[(k * pcells + (size_t)(y / 2) * lw[l + 1] + x / 2) * D + d];
        }
        for (int t = 1; t <= p.iterations; ++t)
            for (int y = 0; y < ch; ++y)
                for (int x = 0; x < cw; ++x) {
                    if ((x + y + t) % 2 == 0) continue;           // the other parity sends
                    const size_t q = (size_t)y * cw + x;
                    for (int k = 0; k < 4; ++k) {
                        // to the neighbour on side k: everything but what came from there, into its slot of the opposite side
                        const int nx = x + from[k][0], ny = y + from[k][1];
                        if (nx < 0 || nx >= cw || ny < 0 || ny >= ch) continue;
                        int low = 0;
                        for (int d = 0; d < D; ++d) {
                            int v = data[l][q * D + d];
                            for (int r = 0; r < 4; ++r)
                                if (r != k) v += msg[(r * cells + q) * D + d];
                            out[d] = v;
                            low = d == 0 || v < low ? v : low;
                        }
                        for (int d = 1; d < D; ++d) out[d] = out[d - 1] + p.step < out[d] ? out[d - 1] + p.step : out[d];
                        for (int d = D - 2; d >= 0; --d) out[d] = out[d + 1] + p.step < out[d] ? out[d + 1] + p.step : out[d];
                        int* dst = &msg[((size_t)(k ^ 1) * cells + (size_t)ny * cw + nx) * D];
                        for (int d = 0; d < D; ++d) dst[d] = (out[d] < low + p.trunc ? out[d] : low + p.trunc) - low;
                    }
                }
        coarse.swap(msg);
    }
    const vector<int>& m0 = coarse;      // (the messages of level 0)
    for (size_t i = 0; i < n; ++i) {
        int z = 0, sz = 0;
        for (int d = 0; d < D; ++d) {
            int s = data[0][i * D + d];
            for (int k = 0; k < 4; ++k) s += m0[(k * n + i) * D + d];
            if (d == 0 || s <= sz) { z = d; sz = s; }            // the last slice of equal beliefs wins
            if (agg) agg[(size_t)d * n + i] = (float)s;
        }
        if (best) best[i] = (float)sz;
        if (disp_map) disp_map[i] = (float)(dmin + z);
    }
}

// ---- scanlineOptimization.cuh (not in the reference) -----------------------------------------
// The scan-line optimiser by the definition in include/smx.h: sgm_aggregateOnCPU with the two edge flags looked up, and the
// penalties chosen, for every pixel, direction and label.
void scanline_optimizeOnCPU(const unsigned char* guide_own, const unsigned char* guide_other, int channels, const float* cost,
                            float* agg, float* best, float* disp_map, const int w, const int h, const int size_d, const int dmin,
                            const smx_scanline_params& p) {
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    const size_t n = (size_t)w * h;
    const int nch = channels < 3 ? channels : 3;
    const int P1[3] = {p.p1, p.p1 / 4, p.p1 / 10}, P2[3] = {p.p2, p.p2 / 4, p.p2 / 10};
    // [D(a, b) >= tau_so] for two pixels of one guide, both inside the image
    auto edge = [&](const unsigned char* g, long long ax, int ay, long long bx, int by) {
        const unsigned char* a = g + ((size_t)ay * w + (size_t)ax) * channels;
        const unsigned char* b = g + ((size_t)by * w + (size_t)bx) * channels;
        int d = 0;
        for (int c = 0; c < nch; ++c) {
            const int e = (int)a[c] - (int)b[c];
            d = (e < 0 ? -e : e) > d ? (e < 0 ? -e : e) : d;
        }
        return d >= p.tau_so ? 1 : 0;
    };
    vector<int> C(n * size_d), L(n * size_d), S(n * size_d, 0);     // [pixel][d]
    for (int d = 0; d < size_d; ++d)
        for (size_t i = 0; i < n; ++i) {
            const float c = cost[(size_t)d * n + i];
            C[i * size_d + d] = c >= 0.0f ? (c <= 255.0f ? (int)c : 255) : 0;
        }
    for (int r = 0; r < p.paths; ++r) {
        const int dx = dirs[r][0], dy = dirs[r][1];
        for (int iy = 0; iy < h; ++iy) {
            const int y = dy >= 0 ? iy : h - 1 - iy;
            for (int ix = 0; ix < w; ++ix) {
                const int x = dx >= 0 ? ix : w - 1 - ix;
                const int px = x - dx, py = y - dy;
                int* cur = &L[((size_t)y * w + x) * size_d];
                const int* c = &C[((size_t)y * w + x) * size_d];
                if (px < 0 || px >= w || py < 0 || py >= h) {
                    for (int d = 0; d < size_d; ++d) cur[d] = c[d];
                } else {
                    const int* prev = &L[((size_t)py * w + px) * size_d];
                    const int e1 = edge(guide_own, x, y, px, py);
                    int m = prev[0];
                    for (int d = 1; d < size_d; ++d) m = prev[d] < m ? prev[d] : m;
                    for (int d = 0; d < size_d; ++d) {
                        // the partner of the label in the other view and its predecessor; py is inside already
                        const long long qx = (long long)x + dmin + d;
                        const int e2 = qx >= 0 && qx < w && qx - dx >= 0 && qx - dx < w ? edge(guide_other, qx, y, qx - dx, py) : 0;
                        const int p1 = P1[e1 + e2], p2 = P2[e1 + e2];
                        int t = prev[d] < m + p2 ? prev[d] : m + p2;
                        if (d - 1 >= 0 && prev[d - 1] + p1 < t) t = prev[d - 1] + p1;
                        if (d + 1 < size_d && prev[d + 1] + p1 < t) t = prev[d + 1] + p1;
                        cur[d] = c[d] + t - m;
                    }
                }
                int* s = &S[((size_t)y * w + x) * size_d];
                for (int d = 0; d < size_d; ++d) s[d] += cur[d];
            }
        }
    }
    for (size_t i = 0; i < n; ++i) {
        const int* s = &S[i * size_d];
        int z = 0;
        for (int d = 1; d < size_d; ++d)
            if (s[d] <= s[z]) z = d;                 // the last slice of equal sums wins
        if (best) best[i] = (float)s[z];
        if (disp_map) disp_map[i] = (float)(dmin + z);
        if (agg)
            for (int d = 0; d < size_d; ++d) agg[(size_t)d * n + i] = (float)s[d];
    }
}
