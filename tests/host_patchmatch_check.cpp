// The CPU twins of PatchMatch stereo (stereo_matching_cuda_amd/host/cpu_twins.cpp: patchMatchOnCPU, pmPlaneCostOnCPU) as a
// stand-alone program, built and run by tests/test_host_patchmatch_cpu.py on the CPU only -- once plain, once under
// -fsanitize=address,undefined -- in the manner of tests/host_adjust_check.cpp.
//
//   host_patchmatch_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, the outputs are written
// beside it.
//   search <stem> w h size_d dminl dminr radius gamma iterations max_slope seed
//        in:  <stem>.left.u8, <stem>.right.u8 (h*w)
//        out: <stem>.planes.f32 (6*h*w), <stem>.cost.f32, <stem>.disp.f32, <stem>.label.f32 (2*h*w each)
//   cost <stem> w h size_d dminl dminr radius gamma iterations max_slope seed
//        in:  the two images and <stem>.planes.f32 (6*h*w)
//        out: <stem>.cost.f32 (2*h*w)
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with the values
// of tests/patchmatch_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "patchMatch.cuh"

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

bool run_case(const std::string& base, std::istringstream& in, bool search) {
    int w, h, D, dminl, dminr;
    unsigned long seed;
    smx_pm_params p;
    if (!(in >> w >> h >> D >> dminl >> dminr >> p.radius >> p.gamma >> p.iterations >> p.max_slope >> seed)) return false;
    p.seed = (uint32_t)seed;
    const size_t n = (size_t)w * h;
    std::vector<unsigned char> left, right;
    if (!read_raw(base + ".left.u8", n, left) || !read_raw(base + ".right.u8", n, right)) return false;
    // 0x7FA00000: a NaN the twins do not write, so that an element left unwritten shows in the comparison
    const uint32_t bits = 0x7FA00000u;
    float unwritten;
    std::memcpy(&unwritten, &bits, 4);
    std::vector<float> planes(6 * n, unwritten), cost(2 * n, unwritten), disp(2 * n, unwritten), label(2 * n, unwritten);
    if (!search) {
        if (!read_raw(base + ".planes.f32", 6 * n, planes)) return false;
        pmPlaneCostOnCPU(left.data(), right.data(), planes.data(), cost.data(), w, h, D, dminl, dminr, p);
        return write_raw(base + ".cost.f32", cost);
    }
    patchMatchOnCPU(left.data(), right.data(), planes.data(), cost.data(), disp.data(), label.data(), w, h, D, dminl, dminr, p);
    return write_raw(base + ".planes.f32", planes) && write_raw(base + ".cost.f32", cost) && write_raw(base + ".disp.f32", disp) &&
           write_raw(base + ".label.f32", label);
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
        if ((stage != "search" && stage != "cost") || !run_case(dir + "/" + stem, in, stage == "search")) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
