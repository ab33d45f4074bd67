// The host arithmetic of the tree filter (stereo_matching_cuda_amd/csrc/smx_tree_host.h: the code the library's entries run) as a
// stand-alone program, built and run by tests/test_tree_cpu.py on the CPU only -- once plain, once under
// -fsanitize=address,undefined.  No libsmx_hip.so, nothing loaded into python.
//
//   host_tree_check <dir>
//
// <dir>/cases.txt holds one case a line:
//   build  <name> <w> <h> <channels>      <name>.guide.u8 in;  <name>.blob.u8 out, in a buffer of exactly tree_layout(w*h).bytes
//   tables <name> <sigma>                 <name>.t.f32 and <name>.u.f32 out
// It prints "cases N" at the end.
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "smx_tree_host.h"

static std::vector<char> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void spill(const std::string& path, const void* p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)p, (std::streamsize)n);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    std::ifstream cases(dir + "/cases.txt");
    std::string line;
    int done = 0;
    while (std::getline(cases, line)) {
        std::istringstream in(line);
        std::string what, name;
        in >> what >> name;
        if (what == "build") {
            int w, h, ch;
            in >> w >> h >> ch;
            const std::vector<char> guide = slurp(dir + "/" + name + ".guide.u8");
            if (guide.size() != (size_t)w * h * ch) return 3;
            const size_t bytes = smx::tree_layout((size_t)w * h).bytes;
            std::unique_ptr<uint32_t[]> blob(new uint32_t[bytes / 4]);      // (exactly as large: a byte too far is a report)
            smx::tree_build((const uint8_t*)guide.data(), ch, w, h, (uint8_t*)blob.get());
            spill(dir + "/" + name + ".blob.u8", blob.get(), bytes);
        } else if (what == "tables") {
            smx_tree_params p;
            in >> p.sigma;
            if (!smx::tree_params_ok(&p)) return 4;
            float t[256], u[256];
            smx::tree_tables(&p, t, u);
            spill(dir + "/" + name + ".t.f32", t, sizeof(t));
            spill(dir + "/" + name + ".u.f32", u, sizeof(u));
        } else return 5;
        ++done;
    }
    std::printf("cases %d\n", done);
    return 0;
}
