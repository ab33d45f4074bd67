// The CPU twins of the opt-in stages (stereo_matching_cuda_amd/host/cpu_twins.cpp: sgm_aggregateOnCPU,
// speckle_filterOnCPU, weighted_medianOnCPU) as a stand-alone program, built and run by tests/test_host_twins_cpu.py on
// the CPU only -- once plain, once under -fsanitize=address,undefined -- the other half of the sanitizer leg of
// tests/host_sanitize_check.cpp (which covers the twins of the reference's own stages).
//
//   host_twins_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, every output is
// written beside it.  f32 parameters are given as the hexadecimal bits of the float, doubles in decimal (17 digits).
//   sgm <stem> w h size_d dmin p1 p2 paths want_agg want_best want_disp
//         in:  <stem>.cost.f32 (size_d*h*w)            out: <stem>.agg.f32, <stem>.best.f32, <stem>.disp.f32
//         an output whose want flag is 0 is passed as nullptr and not written
//   speckle <stem> w h vmin_bits new_val_bits max_size max_diff_bits
//         in:  <stem>.disp.f32 (h*w)                   out: <stem>.out.f32
//   wmf <stem> w h dmin size_d radius sigma_s sigma_c has_select
//         in:  <stem>.guide.u8, <stem>.disp.f32, and with has_select = 1 <stem>.select.f32 (else select = nullptr)
//                                                      out: <stem>.out.f32
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with
// tests/sgm_ref.py, tests/speckle_ref.py and tests/wmf_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "sgm.cuh"
#include "speckle.cuh"
#include "wmf.cuh"

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

bool write_raw(const std::string& path, const std::vector<float>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
    return f.good();
}

float from_bits(const std::string& hex) {
    const uint32_t u = (uint32_t)std::stoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

bool run_sgm(const std::string& base, std::istringstream& in) {
    int w, h, D, dmin, want_agg, want_best, want_disp;
    smx_sgm_params p;
    if (!(in >> w >> h >> D >> dmin >> p.p1 >> p.p2 >> p.paths >> want_agg >> want_best >> want_disp)) return false;
    const size_t n = (size_t)w * h;
    std::vector<float> cost;
    if (!read_raw(base + ".cost.f32", n * D, cost)) return false;
    // 0x7FA00000: a NaN no twin writes, so that an element left unwritten shows in the comparison
    std::vector<float> agg(want_agg ? n * D : 0, from_bits("7FA00000")), best(want_best ? n : 0, from_bits("7FA00000")),
        disp(want_disp ? n : 0, from_bits("7FA00000"));
    sgm_aggregateOnCPU(cost.data(), want_agg ? agg.data() : nullptr, want_best ? best.data() : nullptr,
                       want_disp ? disp.data() : nullptr, w, h, D, dmin, p);
    return (!want_agg || write_raw(base + ".agg.f32", agg)) && (!want_best || write_raw(base + ".best.f32", best)) &&
           (!want_disp || write_raw(base + ".disp.f32", disp));
}

bool run_speckle(const std::string& base, std::istringstream& in) {
    int w, h;
    std::string vmin, new_val, max_diff;
    smx_speckle_params p;
    if (!(in >> w >> h >> vmin >> new_val >> p.max_size >> max_diff)) return false;
    p.max_diff = from_bits(max_diff);
    const size_t n = (size_t)w * h;
    std::vector<float> disp;
    if (!read_raw(base + ".disp.f32", n, disp)) return false;
    std::vector<float> out(n, from_bits("7FA00000"));
    speckle_filterOnCPU(disp.data(), out.data(), w, h, from_bits(vmin), from_bits(new_val), p);
    return write_raw(base + ".out.f32", out);
}

bool run_wmf(const std::string& base, std::istringstream& in) {
    int w, h, dmin, size_d, has_select;
    smx_wmf_params p;
    if (!(in >> w >> h >> dmin >> size_d >> p.radius >> p.sigma_s >> p.sigma_c >> has_select)) return false;
    const size_t n = (size_t)w * h;
    std::vector<unsigned char> guide;
    std::vector<float> disp, select;
    if (!read_raw(base + ".guide.u8", n, guide) || !read_raw(base + ".disp.f32", n, disp)) return false;
    if (has_select && !read_raw(base + ".select.f32", n, select)) return false;
    std::vector<float> out(n, from_bits("7FA00000"));
    weighted_medianOnCPU(guide.data(), disp.data(), has_select ? select.data() : nullptr, out.data(), w, h, dmin, size_d, p);
    return write_raw(base + ".out.f32", out);
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
        const bool ok = stage == "sgm" ? run_sgm(base, in) : stage == "speckle" ? run_speckle(base, in) :
                        stage == "wmf" ? run_wmf(base, in) : false;
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
