// The CPU twin of the AD-Census cost (stereo_matching_cuda_amd/host/cpu_twins.cpp: adcensus_costOnCPU) as a stand-alone
// program, built and run by tests/test_host_adcensus_cpu.py on the CPU only -- once plain, once under
// -fsanitize=address,undefined -- like tests/host_twins_check.cpp for the twins of the other opt-in stages.
//
//   host_adcensus_check DIR
//
// DIR/cases.txt lists one case per line; every file is raw little-endian, DIR/<stem>.<name>:
//   <stem> w h size_d dmin channels rx ry th colour
//         <stem>.i1.u8, <stem>.i2.u8 (h*w*channels): the images of the absolute differences;  <stem>.g1.u8, <stem>.g2.u8
//         (h*w): the gray images of the census codes;  <stem>.table.f32 (SMX_ADCENSUS_TABLE_FLOATS): the tables of
//         smx_adcensus_tables;  <stem>.want.f32 (size_d*h*w): the volume of tests/adcensus_ref.py
// The twin's volume is compared with <stem>.want.f32 bit for bit: `ok <stem>` or `MISMATCH <stem> ...` per case, `cases
// <count>` at the end; exit 1 on a mismatch or a case it cannot read.
// No GPU, no libsmx_hip.so, no oracle: the symbols the twins need from the host layer are defined here.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "adcensus.cuh"

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

// 1 the twin equals the reference, 0 it does not, -1 the case cannot be read
int run_case(const std::string& base, const std::string& stem, std::istringstream& in) {
    int w, h, D, dmin, ch;
    smx_adcensus_params p;
    p.lambda_census = p.lambda_ad = p.scale = 0.0;     // (the twin reads the tables, not these)
    if (!(in >> w >> h >> D >> dmin >> ch >> p.census.rx >> p.census.ry >> p.census.th >> p.colour)) return -1;
    const size_t n = (size_t)w * h;
    std::vector<unsigned char> i1, i2, g1, g2;
    std::vector<float> table, want;
    if (!read_raw(base + ".i1.u8", n * ch, i1) || !read_raw(base + ".i2.u8", n * ch, i2) || !read_raw(base + ".g1.u8", n, g1) ||
        !read_raw(base + ".g2.u8", n, g2) || !read_raw(base + ".table.f32", (size_t)SMX_ADCENSUS_TABLE_FLOATS, table) ||
        !read_raw(base + ".want.f32", n * D, want))
        return -1;
    uint32_t unwritten = 0x7FA00000u;                  // a NaN the twin never writes: an element left out shows
    float fill;
    std::memcpy(&fill, &unwritten, 4);
    std::vector<float> got(n * D, fill);
    adcensus_costOnCPU(i1.data(), i2.data(), g1.data(), g2.data(), ch, got.data(), w, h, D, dmin, p, table.data());
    for (size_t k = 0; k < got.size(); ++k)
        if (std::memcmp(&got[k], &want[k], 4) != 0) {
            std::printf("MISMATCH %s first at %zu: twin %a, reference %a\n", stem.c_str(), k, (double)got[k], (double)want[k]);
            return 0;
        }
    std::printf("ok %s\n", stem.c_str());
    return 1;
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
    int count = 0, bad = 0;
    for (std::string line; std::getline(list, line);) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string stem;
        in >> stem;
        const int rc = run_case(dir + "/" + stem, stem, in);
        if (rc < 0) {
            std::fprintf(stderr, "cannot run the case `%s`\n", line.c_str());
            return 1;
        }
        bad += rc == 0;
        ++count;
    }
    std::printf("cases %d\n", count);
    return bad ? 1 : 0;
}
