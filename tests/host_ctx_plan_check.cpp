// The persistent context's rules (stereo_matching_cuda_amd/csrc/smx_ctx_plan.h: the stage table and plan_pair) as a stand-alone
// program, built and run by tests/test_ctx_plan_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined.
//
//   host_ctx_plan_check DIR
//
// A point is a key and a call.  The key: bits 0-1 the cost (0 reference, 1 census, 2 AD-Census gray, 3 AD-Census colour), bits
// 2-14 on / off for SGM, colour guidance, cross, scan-line, cross-scale, permeability, bp, PatchMatch, adjust, uniqueness,
// sub-pixel, speckle, vote, bits 15-17 mean images / cost volumes / aggregated volumes wanted.  The call: the entry (0 gray,
// 1 rgb, 2 async), channels, w, h, size_d, dminl, dminr.
// It writes, as raw little-endian int32:
//   DIR/full.i32    the whole key space, 2^18 keys on the gray entry and then 2^18 on the rgb entry with 3 channels, at
//                   16 x 8 x 4 with dmin -3 / 0
//   DIR/extra.i32   the points of DIR/extra.txt (one per line: key entry channels w h size_d dminl dminr), in its order
// with four values per point: the verdict, the plan's bits (cost agg subpix census sgm speckle uniq cgf cross vote so adjust
// cscale level pm perm bp walker_status from bit 0), the message's line in DIR/messages.txt or -1, and stages_on().
// DIR/table.txt is the stage table: index, setter, excludes, no_mean, checked, noun, shapes, tab-separated.
// The program decides nothing: every comparison with tests/ctx_plan_ref.py is the test's.  It exits 1 on a line it cannot read.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "smx_ctx_plan.h"

using namespace smx;

static CtxSettings settings_of(unsigned key) {
    CtxSettings s;
    const unsigned cost = key & 3;
    auto b = [key](int i) { return (key >> i & 1) != 0; };
    s.cost_mode = cost == 1 ? SMX_COST_CENSUS : SMX_COST_REFERENCE;
    s.adcensus = cost >= 2;
    s.adc = {};
    s.adc.colour = cost == 3;
    s.agg_mode = b(2) ? SMX_AGG_SGM : SMX_AGG_GUIDED;
    s.guide_mode = b(3) ? SMX_GUIDE_RGB : SMX_GUIDE_GRAY;
    s.cross = b(4); s.so = b(5); s.cscale = b(6); s.perm = b(7); s.bp = b(8); s.pm = b(9); s.adjust = b(10);
    s.uniq = b(11) ? 0.15f : 0.0f;
    s.subpix = b(12) ? SMX_SUBPIX_PARABOLA : 0;
    s.speckle = b(13); s.vote = b(14);
    return s;
}

struct Out {
    std::vector<int32_t> rec;
    std::map<std::string, int>* ids;
    std::vector<std::string>* msgs;
    void point(unsigned key, int entry, int channels, int w, int h, int size_d, int dminl, int dminr) {
        const CtxSettings s = settings_of(key);
        PairPlan p;
        char err[512] = "";
        const int rc = plan_pair(s, w, h, size_d, (PairEntry)entry, channels, dminl, dminr, key >> 16 & 1, key >> 17 & 1, key >> 15 & 1,
                                 &p, err, sizeof(err));
        const bool bits[18] = {p.cost, p.agg, p.subpix, p.census, p.sgm, p.speckle, p.uniq, p.cgf, p.cross, p.vote, p.so, p.adjust,
                               p.cscale, p.level, p.pm, p.perm, p.bp, p.walker_status};
        int32_t plan = 0, id = -1;
        for (int i = 0; i < 18; ++i) plan |= bits[i] ? 1 << i : 0;
        if (rc != SMX_OK) {
            auto it = ids->find(err);
            if (it == ids->end()) { it = ids->emplace(err, (int)msgs->size()).first; msgs->push_back(err); }
            id = it->second;
        }
        rec.insert(rec.end(), {rc, plan, id, (int32_t)stages_on(s)});
    }
    bool write(const std::string& path) const {
        std::ofstream f(path, std::ios::binary);
        f.write((const char*)rec.data(), (std::streamsize)(rec.size() * sizeof(int32_t)));
        return (bool)f;
    }
};

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: host_ctx_plan_check DIR\n"); return 1; }
    const std::string dir = argv[1];
    std::map<std::string, int> ids;
    std::vector<std::string> msgs;
    Out full{{}, &ids, &msgs}, extra{{}, &ids, &msgs};
    for (int entry = 0; entry < 2; ++entry)
        for (unsigned key = 0; key < (1u << 18); ++key) full.point(key, entry, entry ? 3 : 0, 16, 8, 4, -3, 0);
    std::ifstream in(dir + "/extra.txt");
    std::string line;
    int lines = 0;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        unsigned key;
        int entry, channels, w, h, size_d, dminl, dminr;
        if (!(ss >> key >> entry >> channels >> w >> h >> size_d >> dminl >> dminr) || entry < 0 || entry > 2) {
            std::printf("cannot read line %d of extra.txt\n", lines + 1);
            return 1;
        }
        extra.point(key, entry, channels, w, h, size_d, dminl, dminr);
        ++lines;
    }
    std::ofstream table(dir + "/table.txt");
    for (int i = 0; i < N_STAGES; ++i) {
        const StageRow& r = STAGES[i];
        table << i << '\t' << r.setter << '\t' << r.excludes << '\t' << ((r.flags & NO_MEAN) != 0) << '\t' << r.limit.checked << '\t' << r.noun << '\t'
              << (r.limit.shapes ? r.limit.shapes : "") << '\n';
    }
    std::ofstream m(dir + "/messages.txt");
    for (const std::string& s : msgs) m << s << '\n';
    if (!full.write(dir + "/full.i32") || !extra.write(dir + "/extra.i32") || !table || !m) { std::printf("cannot write to %s\n", dir.c_str()); return 1; }
    std::printf("points %zu extra %d messages %zu\n", full.rec.size() / 4, lines, msgs.size());
    return 0;
}
