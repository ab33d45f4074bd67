// The CPU twin of region voting (stereo_matching_cuda_amd/host/cpu_twins.cpp: region_voteOnCPU) as a stand-alone program, built
// and run by tests/test_host_vote_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined -- in the manner
// of tests/host_cross_check.cpp.
//
//   host_vote_check DIR
//
// DIR/cases.txt lists one case per line; every input is a raw little-endian file DIR/<stem>.<name>, the output is written
// beside it.
//   vote <stem> w h channels size_d dmin d_lr tau_s tau_h_pct iterations interpolate l1 l2 tau1 tau2 have_right
//        in:  <stem>.guide.u8 (h*w*channels), <stem>.disp.f32 (h*w), and with have_right = 1 <stem>.right.f32 (h*w; else NULL)
//        out: <stem>.voted.f32 (h*w)
// The program decides nothing: it prints `ran <stem>` per case and `cases <count>` at the end; the comparison with the values
// of tests/vote_ref.py is the test's.  It exits 1 on a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "regionVoting.cuh"

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

bool run_vote(const std::string& base, std::istringstream& in) {
    int w, h, channels, D, dmin, d_lr, have_right;
    smx_vote_params p;
    smx_cross_params arms;
    arms.iterations = 1;
    if (!(in >> w >> h >> channels >> D >> dmin >> d_lr >> p.tau_s >> p.tau_h_pct >> p.iterations >> p.interpolate >> arms.l1 >>
          arms.l2 >> arms.tau1 >> arms.tau2 >> have_right))
        return false;
    const size_t n = (size_t)w * h;
    std::vector<unsigned char> guide;
    std::vector<float> disp, right;
    if (!read_raw(base + ".guide.u8", n * channels, guide) || !read_raw(base + ".disp.f32", n, disp)) return false;
    if (have_right && !read_raw(base + ".right.f32", n, right)) return false;
    // 0x7FA00000: a NaN the twin does not write, so that an element left unwritten shows in the comparison
    const uint32_t bits = 0x7FA00000u;
    float unwritten;
    std::memcpy(&unwritten, &bits, 4);
    std::vector<float> out(n, unwritten);
    smx_config().params.d_lr = d_lr;
    region_voteOnCPU(guide.data(), channels, disp.data(), have_right ? right.data() : nullptr, out.data(), w, h, dmin, D, p, arms);
    return write_raw(base + ".voted.f32", out);
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
        if (stage != "vote" || !run_vote(dir + "/" + stem, in)) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        std::printf("ran %s\n", stem.c_str());
        ++count;
    }
    std::printf("cases %d\n", count);
    return 0;
}
