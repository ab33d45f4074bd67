// The CPU twin of the depth-discontinuity adjustment (stereo_matching_cuda_amd/host/cpu_twins.cpp: discontinuityAdjustOnCPU) as a
// stand-alone program, built and run by tests/test_host_adjust_cpu.py on the CPU only -- once plain, once under
// -fsanitize=address,undefined -- in the manner of tests/host_vote_check.cpp.
//
//   host_adjust_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, the outputs are written
// beside it.
//   adjust <stem> w h size_d dmin tau_e vertical iterations subpix_mode
//        in:  <stem>.disp.f32 (h*w), <stem>.agg.f32 (size_d*h*w), and with subpix_mode != 0 <stem>.sub.f32 (h*w; else NULL)
//        out: <stem>.adjusted.f32 (h*w), and with subpix_mode != 0 <stem>.subout.f32 (h*w)
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with the values
// of tests/adjust_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "discontinuityAdjustment.cuh"

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

bool run_adjust(const std::string& base, std::istringstream& in) {
    int w, h, D, dmin, mode;
    smx_adjust_params p;
    if (!(in >> w >> h >> D >> dmin >> p.tau_e >> p.vertical >> p.iterations >> mode)) return false;
    const size_t n = (size_t)w * h;
    std::vector<float> disp, agg, sub;
    if (!read_raw(base + ".disp.f32", n, disp) || !read_raw(base + ".agg.f32", n * D, agg)) return false;
    if (mode && !read_raw(base + ".sub.f32", n, sub)) return false;
    // 0x7FA00000: a NaN the twin does not write, so that an element left unwritten shows in the comparison
    const uint32_t bits = 0x7FA00000u;
    float unwritten;
    std::memcpy(&unwritten, &bits, 4);
    std::vector<float> out(n, unwritten);
    discontinuityAdjustOnCPU(disp.data(), agg.data(), out.data(), w, h, dmin, D, p, mode, mode ? sub.data() : nullptr);
    return write_raw(base + ".adjusted.f32", out) && (!mode || write_raw(base + ".subout.f32", sub));
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
        if (stage != "adjust" || !run_adjust(dir + "/" + stem, in)) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
