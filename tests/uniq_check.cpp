// The CPU twin of the uniqueness filter (stereo_matching_cuda_amd/host/cpu_twins.cpp: uniqueness_onCPU) as a stand-alone
// program, built and run by tests/test_uniq_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined.
//
//   uniq_check DIR
//
// DIR/cases.txt lists one case per line; f32 parameters are given as the hexadecimal bits of the float.
//   uniq <stem> w h size_d ratio_bits vmin_bits new_val_bits want_margin
//         in:  <stem>.agg.f32 (size_d*h*w), <stem>.disp.f32 (h*w)      out: <stem>.out.f32, <stem>.margin.f32
//         with want_margin = 0 the margin is passed as nullptr and not written
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with
// tests/uniq_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "uniqueness.cuh"

bool check_errors(unsigned char* a, unsigned char* b, int len) { return std::memcmp(a, b, (size_t)len) == 0; }
bool check_errors(float* a, float* b, int len) { return std::memcmp(a, b, (size_t)len * 4) == 0; }

smx_host_config& smx_config() {
    static smx_host_config c = {{0.299, 0.587, 0.0721, 0.9, 7, 2, 9, 6.5025, 0}, -5, 0};
    return c;
}

namespace {

bool read_raw(const std::string& path, size_t count, std::vector<float>& out) {
    std::ifstream f(path, std::ios::binary);
    const std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() != count * sizeof(float)) {
        std::fprintf(stderr, "%s: %zu bytes, expected %zu\n", path.c_str(), raw.size(), count * sizeof(float));
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
        std::string stage, stem, ratio, vmin, new_val;
        int w, h, D, want_margin;
        if (!(in >> stage >> stem >> w >> h >> D >> ratio >> vmin >> new_val >> want_margin) || stage != "uniq") {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        const std::string base = dir + "/" + stem;
        const size_t n = (size_t)w * h;
        std::vector<float> agg, disp;
        if (!read_raw(base + ".agg.f32", n * D, agg) || !read_raw(base + ".disp.f32", n, disp)) return 1;
        // 0x7FA00000: a NaN the twin never writes, so that an element left unwritten shows in the comparison
        std::vector<float> out(n, from_bits("7FA00000")), margin(want_margin ? n : 0, from_bits("7FA00000"));
        uniqueness_onCPU(agg.data(), disp.data(), out.data(), want_margin ? margin.data() : nullptr, w, h, D, from_bits(ratio),
                         from_bits(vmin), from_bits(new_val));
        if (!write_raw(base + ".out.f32", out) || (want_margin && !write_raw(base + ".margin.f32", margin))) return 1;
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
