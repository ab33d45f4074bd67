/*
 * ref_driver.cpp -- our own main() in front of the reference's host functions.  TEST INFRASTRUCTURE ONLY.
 *
 * oracle/ref_build.py compiles it against a temporary copy of the reference (one build per set of the macros of
 * SystemIncludes.h) and the host stand-in of oracle/ref_shim.  It reads raw little-endian arrays from a directory, calls
 * rgb_to_grayscale / compute_cost / compute_guided_filter / detect_occlusion / fill_occlusion / write_mat, and writes raw arrays
 * back.
 *
 *   ref_<variant> pair <dir> <w> <h> [channels]
 *       in : left.u8 right.u8          gray [h][w], or interleaved RGB(A) when channels is 3 or 4
 *       out: I_l.u8 I_r.u8 costl.f32 costr.f32 mean1.u8 mean2.u8 best_costl.f32 best_costr.f32 dmapl.f32 dmapr.f32
 *            occlusion.f32 occlusion_filled.f32 aggl.f32 aggr.f32     (the sequence of main.cu:65-155)
 *   ref_<variant> gf <dir> <w> <h> <size_d> <dmin>
 *       in : I.u8 cost.f32 [size_d][h][w], best.f32 dmap.f32 (the in/out presets)
 *       out: best_out.f32 dmap_out.f32 mean.u8 agg.f32
 *   ref_<variant> occ <dir> <w> <h> <dOcclusion> <vMin>
 *       in : dl.f32, optionally dr.f32 (with it: detect_occlusion first)
 *       out: occlusion.f32 (only with dr.f32), filled.f32
 *   ref_<variant> gray <dir> <n> <channels>
 *       in : rgb.u8      out: gray.u8
 *   ref_<variant> wm <dir> <n>
 *       in : mat.f32     out: mat.u8   (the bytes write_mat hands to the PNG writer, main.cu:32)
 */
#include "rgb_to_grayscale.cuh"
#include "costVolume.cuh"
#include "guidedFilter.cuh"
#include "occlusion.cuh"

#include <string>
#include <vector>

/* main.cu:13 -- no header of the reference declares it; ref_build.py cuts its text into a unit of its own */
void write_mat(float* mat, const char* filename, int w, int h, int start);

static std::string g_dir;

static std::string path_of(const char* name) { return g_dir + "/" + name; }

static bool exists(const char* name) {
    FILE* f = fopen(path_of(name).c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

template <class T> static T* slurp(const char* name, size_t count) {
    FILE* f = fopen(path_of(name).c_str(), "rb");
    if (!f) { fprintf(stderr, "ref_driver: cannot open %s\n", name); exit(2); }
    T* p = (T*)malloc(count * sizeof(T));      /* exact size: a host sanitizer sees a read past the end */
    size_t got = fread(p, sizeof(T), count, f);
    bool more = fgetc(f) != EOF;
    fclose(f);
    if (got != count || more) { fprintf(stderr, "ref_driver: %s does not hold %zu elements\n", name, count); exit(2); }
    return p;
}

template <class T> static void dump(const char* name, const T* p, size_t count) {
    FILE* f = fopen(path_of(name).c_str(), "wb");
    if (!f || fwrite(p, sizeof(T), count, f) != count) { fprintf(stderr, "ref_driver: cannot write %s\n", name); exit(2); }
    fclose(f);
}

static void capture_to(const char* name) {
    if (ref_capture_file) fclose(ref_capture_file);
    ref_capture_file = name ? fopen(path_of(name).c_str(), "wb") : nullptr;
    if (name && !ref_capture_file) { fprintf(stderr, "ref_driver: cannot write %s\n", name); exit(2); }
}

/* The call sequence of main.cu:65-155: gray conversion, both cost volumes (right view: dmin = -D_MAX, images swapped), both
 * aggregations from the presets main() gives them, the left-right check on a copy of the left map, the filling of a copy. */
static int run_pair(int w, int h, int channels) {
    const int n = w * h;
    const int slices = D_MAX - D_MIN + 1;
    const int dmin_left = D_MIN, dmin_right = -D_MAX;
    unsigned char* gray[2];
    const char* in_name[2] = {"left.u8", "right.u8"};
    for (int v = 0; v < 2; ++v) {
        if (channels >= 3) {
            unsigned char* rgb = slurp<unsigned char>(in_name[v], (size_t)n * channels);
            gray[v] = rgb_to_grayscale(rgb, n, channels, false);
            free(rgb);
        } else {
            gray[v] = slurp<unsigned char>(in_name[v], n);
        }
    }
    std::vector<float> cost[2], best[2], dmap[2];
    std::vector<unsigned char> mean[2], unused[2];
    /* main() presets the best-cost planes with memset(p, 9999999.0f, bytes): the float converts to int, memset keeps its low
     * byte.  The same conversion here, so the planes start from the same bytes whatever they are. */
    const int preset = (int)9999999.0f;
    for (int v = 0; v < 2; ++v) {
        cost[v].assign((size_t)n * slices, 0.0f);
        best[v].resize(n);
        memset(best[v].data(), preset, sizeof(float) * n);
        dmap[v].assign(n, 0.0f);
        mean[v].assign(n, 0);
        unused[v].assign(n, 0);
    }
    compute_cost(gray[0], gray[1], cost[0].data(), w, w, h, h, dmin_left, false);
    compute_cost(gray[1], gray[0], cost[1].data(), w, w, h, h, dmin_right, false);
    const char* agg_name[2] = {"aggl.f32", "aggr.f32"};
    for (int v = 0; v < 2; ++v) {
        capture_to(agg_name[v]);
        compute_guided_filter(gray[v], cost[v].data(), best[v].data(), dmap[v].data(), mean[v].data(), w, h, slices,
                              v == 0 ? dmin_left : dmin_right, false);
    }
    capture_to(nullptr);
    std::vector<float> occ(dmap[0]);
    detect_occlusion(occ.data(), dmap[1].data(), dmin_left - 100, unused[0].data(), unused[1].data(), w, h);
    std::vector<float> filled(occ);
    const int v_min = D_MIN;                       /* an int in main(), converted to the float parameter */
    fill_occlusion(filled.data(), w, h, v_min);

    dump("I_l.u8", gray[0], n); dump("I_r.u8", gray[1], n);
    dump("costl.f32", cost[0].data(), cost[0].size()); dump("costr.f32", cost[1].data(), cost[1].size());
    dump("mean1.u8", mean[0].data(), n); dump("mean2.u8", mean[1].data(), n);
    dump("best_costl.f32", best[0].data(), n); dump("best_costr.f32", best[1].data(), n);
    dump("dmapl.f32", dmap[0].data(), n); dump("dmapr.f32", dmap[1].data(), n);
    dump("occlusion.f32", occ.data(), n); dump("occlusion_filled.f32", filled.data(), n);
    free(gray[0]); free(gray[1]);
    return 0;
}

static int run_gf(int w, int h, int size_d, int dmin) {
    const int n = w * h;
    unsigned char* I = slurp<unsigned char>("I.u8", n);
    float* cost = slurp<float>("cost.f32", (size_t)n * size_d);
    float* best = slurp<float>("best.f32", n);
    float* dmap = slurp<float>("dmap.f32", n);
    unsigned char* mean = (unsigned char*)malloc(n);
    memset(mean, 0, n);
    capture_to("agg.f32");
    compute_guided_filter(I, cost, best, dmap, mean, w, h, size_d, dmin, false);
    capture_to(nullptr);
    dump("best_out.f32", best, n); dump("dmap_out.f32", dmap, n); dump("mean.u8", mean, n);
    free(I); free(cost); free(best); free(dmap); free(mean);
    return 0;
}

static int run_occ(int w, int h, int dOcclusion, float vMin) {
    const int n = w * h;
    float* d = slurp<float>("dl.f32", n);
    if (exists("dr.f32")) {
        float* dr = slurp<float>("dr.f32", n);
        unsigned char* cl = (unsigned char*)malloc(n);
        unsigned char* cr = (unsigned char*)malloc(n);
        memset(cl, 0, n);
        memset(cr, 0, n);
        detect_occlusion(d, dr, dOcclusion, cl, cr, w, h);
        dump("occlusion.f32", d, n);
        free(dr); free(cl); free(cr);
    }
    fill_occlusion(d, w, h, vMin);
    dump("filled.f32", d, n);
    free(d);
    return 0;
}

static int run_gray(int n, int channels) {
    unsigned char* rgb = slurp<unsigned char>("rgb.u8", (size_t)n * channels);
    unsigned char* gray = rgb_to_grayscale(rgb, n, channels, false);
    dump("gray.u8", gray, n);
    free(rgb); free(gray);
    return 0;
}

static int run_wm(int n) {
    float* mat = slurp<float>("mat.f32", n);
    capture_to("mat.u8");
    write_mat(mat, "mat.u8", n, 1, 0);
    capture_to(nullptr);
    free(mat);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s pair|gf|occ|gray|wm <dir> ...\n", argv[0]); return 2; }
    const std::string mode = argv[1];
    g_dir = argv[2];
    std::vector<double> a;
    for (int i = 3; i < argc; ++i) a.push_back(atof(argv[i]));
    if (mode == "pair" && a.size() >= 2) return run_pair((int)a[0], (int)a[1], a.size() > 2 ? (int)a[2] : 1);
    if (mode == "gf" && a.size() == 4) return run_gf((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
    if (mode == "occ" && a.size() == 4) return run_occ((int)a[0], (int)a[1], (int)a[2], (float)a[3]);
    if (mode == "gray" && a.size() == 2) return run_gray((int)a[0], (int)a[1]);
    if (mode == "wm" && a.size() == 1) return run_wm((int)a[0]);
    fprintf(stderr, "ref_driver: bad arguments for mode %s\n", mode.c_str());
    return 2;
}
