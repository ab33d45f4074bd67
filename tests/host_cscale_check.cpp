// The CPU twins of cross-scale aggregation (stereo_matching_cuda_amd/host/cpu_twins.cpp: pyrDownOnCPU, crossScaleOnCPU) and the
// host arithmetic behind smx_cscale_weights / smx_cscale_level (csrc/smx_cscale_host.h) as a stand-alone program, built and run
// by tests/test_host_cscale_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined -- in the manner of
// tests/host_adjust_check.cpp.
//
//   host_cscale_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, the outputs are written
// beside it.
//   pyr <stem> w h channels
//        in:  <stem>.src.u8 (h*w*channels)           out: <stem>.dst.u8
//   weights <stem> scales lambda
//        out: <stem>.wt.f32 (scales)
//   combine <stem> w h dmin size_d scales lambda
//        in:  <stem>.level<s>.f32 for s = 0 .. scales-1, the geometry of smx_cscale_level
//        out: <stem>.out.f32 (size_d*h*w), <stem>.best.f32, <stem>.disp.f32 (h*w)
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with the values
// of tests/cscale_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "crossScale.cuh"
#include "../stereo_matching_cuda_amd/csrc/smx_cscale_host.h"

// helpers.cuh (defined in stages.cpp next to the GPU wrappers): exact compare, like helpers.cu:3-25
bool check_errors(unsigned char* a, unsigned char* b, int len) { return std::memcmp(a, b, (size_t)len) == 0; }
bool check_errors(float* a, float* b, int len) { return std::memcmp(a, b, (size_t)len * 4) == 0; }

smx_host_config& smx_config() {
    static smx_host_config c = {{0.299, 0.587, 0.0721, 0.9, 7, 2, 9, 6.5025, 0}, -5, 0};
    return c;
}

namespace {

template <class T>
bool read_raw(const std::string& path, size_t count, std::vector<T>& out) {
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (!f.good() && !f.eof()) return false;
    if (raw.size() != count * sizeof(T)) {
        std::fprintf(stderr, "%s: %zu bytes, expected %zu\n", path.c_str(), raw.size(), count * sizeof(T));
        return false;
    }
    out.resize(count);
    if (count) std::memcpy(out.data(), raw.data(), raw.size());
    return true;
}

template <class T>
bool write_raw(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    return f.good();
}

// 0x7FA00000: a NaN the twins do not write, so that an element left unwritten shows in the comparison
float unwritten() {
    const uint32_t bits = 0x7FA00000u;
    float v;
    std::memcpy(&v, &bits, 4);
    return v;
}

bool run_pyr(const std::string& base, std::istringstream& in) {
    int w, h, ch;
    if (!(in >> w >> h >> ch)) return false;
    std::vector<unsigned char> src;
    if (!read_raw(base + ".src.u8", (size_t)w * h * ch, src)) return false;
    std::vector<unsigned char> dst((size_t)((w + 1) / 2) * ((h + 1) / 2) * ch, 0xA5);
    pyrDownOnCPU(src.data(), dst.data(), w, h, ch);
    return write_raw(base + ".dst.u8", dst);
}

bool run_weights(const std::string& base, std::istringstream& in) {
    smx_cscale_params p;
    if (!(in >> p.scales >> p.lambda) || !smx::cscale_params_ok(&p)) return false;
    std::vector<float> wt((size_t)p.scales, unwritten());
    smx::cscale_weights(&p, wt.data());
    return write_raw(base + ".wt.f32", wt);
}

bool run_combine(const std::string& base, std::istringstream& in) {
    int w, h, dmin, D;
    smx_cscale_params p;
    if (!(in >> w >> h >> dmin >> D >> p.scales >> p.lambda) || !smx::cscale_params_ok(&p)) return false;
    std::vector<std::vector<float>> levels((size_t)p.scales);
    const float* ptrs[SMX_CSCALE_MAX_SCALES] = {};
    for (int s = 0; s < p.scales; ++s) {
        int ws, hs, lo, ds;
        smx::cscale_level(w, h, dmin, D, s, &ws, &hs, &lo, &ds);
        if (!read_raw(base + ".level" + std::to_string(s) + ".f32", (size_t)ws * hs * ds, levels[(size_t)s])) return false;
        ptrs[s] = levels[(size_t)s].data();
    }
    const size_t n = (size_t)w * h;
    std::vector<float> out(n * D, unwritten()), best(n, unwritten()), disp(n, unwritten());
    crossScaleOnCPU(ptrs, out.data(), best.data(), disp.data(), w, h, dmin, D, p);
    return write_raw(base + ".out.f32", out) && write_raw(base + ".best.f32", best) && write_raw(base + ".disp.f32", disp);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s DIR\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    std::ifstream list(dir + "/cases.txt");
    if (!list) {
        std::fprintf(stderr, "cannot read %s/cases.txt\n", dir.c_str());
        return 1;
    }
    int count = 0;
    for (std::string line; std::getline(list, line);) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string stage, stem;
        in >> stage >> stem;
        const std::string base = dir + "/" + stem;
        const bool ok = stage == "pyr" ? run_pyr(base, in) : stage == "weights" ? run_weights(base, in)
                        : stage == "combine" ? run_combine(base, in) : false;
        if (!ok) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
