// The CPU twin of the scan-line optimiser (stereo_matching_cuda_amd/host/cpu_twins.cpp: scanline_optimizeOnCPU) as a stand-alone
// program, built and run by tests/test_host_scanline_cpu.py on the CPU only -- once plain, once under
// -fsanitize=address,undefined -- in the manner of tests/host_vote_check.cpp.
//
//   host_scanline_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, the outputs are written
// beside them.
//   scanline <stem> w h channels size_d dmin p1 p2 tau_so paths want_agg
//        in:  <stem>.own.u8, <stem>.other.u8 (h*w*channels each), <stem>.cost.f32 (size_d*h*w)
//        out: <stem>.best.f32, <stem>.disp.f32 (h*w each), and with want_agg = 1 <stem>.agg.f32 (size_d*h*w; else NULL goes in)
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with the values
// of tests/scanline_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "scanlineOptimization.cuh"

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

bool run_scanline(const std::string& base, std::istringstream& in) {
    int w, h, channels, D, dmin, want_agg;
    smx_scanline_params p;
    if (!(in >> w >> h >> channels >> D >> dmin >> p.p1 >> p.p2 >> p.tau_so >> p.paths >> want_agg)) return false;
    const size_t n = (size_t)w * h;
    std::vector<unsigned char> own, other;
    std::vector<float> cost;
    if (!read_raw(base + ".own.u8", n * channels, own) || !read_raw(base + ".other.u8", n * channels, other) ||
        !read_raw(base + ".cost.f32", n * D, cost))
        return false;
    // 0x7FA00000: a NaN the twin does not write, so that an element left unwritten shows in the comparison
    const uint32_t bits = 0x7FA00000u;
    float unwritten;
    std::memcpy(&unwritten, &bits, 4);
    std::vector<float> best(n, unwritten), disp(n, unwritten), agg(want_agg ? n * D : 0, unwritten);
    scanline_optimizeOnCPU(own.data(), other.data(), channels, cost.data(), want_agg ? agg.data() : nullptr, best.data(),
                           disp.data(), w, h, D, dmin, p);
    return write_raw(base + ".best.f32", best) && write_raw(base + ".disp.f32", disp) && (!want_agg || write_raw(base + ".agg.f32", agg));
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
        if (stage != "scanline" || !run_scanline(dir + "/" + stem, in)) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
