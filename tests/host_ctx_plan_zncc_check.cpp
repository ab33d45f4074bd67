// The ZNCC cost in the persistent context's rules (stereo_matching_cuda_amd/csrc/smx_ctx_plan.h): a fourth value of
// the cost mode that turns on the census cost's row of the stage table under its own name.  A stand-alone program, built and run
// by tests/test_ctx_plan_zncc_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined.
//
//   host_ctx_plan_zncc_check
//
// It walks every combination of the thirteen other stages (bits 0-12: SGM, colour guidance, cross, scan-line, cross-scale,
// permeability, bp, PatchMatch, adjust, uniqueness, sub-pixel, speckle, vote) and of the wanted outputs (bits 13-15: mean images,
// cost volumes, aggregated volumes) on the three entries, once with SMX_COST_CENSUS and once with SMX_COST_ZNCC, and counts the
// points where the two differ in the verdict, in any bit of the plan or in stages_on(), and the refused points whose message is
// not the census mode's with the noun and the setter replaced.  Then it prints the messages of three refusals.
#include <cstdio>
#include <cstring>
#include <string>

#include "smx_ctx_plan.h"

using namespace smx;

static CtxSettings settings_of(unsigned key, int cost_mode) {
    CtxSettings s;
    auto b = [key](int i) { return (key >> i & 1) != 0; };
    s.cost_mode = cost_mode;
    s.zncc = {3, 3};
    s.agg_mode = b(0) ? SMX_AGG_SGM : SMX_AGG_GUIDED;
    s.guide_mode = b(1) ? SMX_GUIDE_RGB : SMX_GUIDE_GRAY;
    s.cross = b(2); s.so = b(3); s.cscale = b(4); s.perm = b(5); s.bp = b(6); s.pm = b(7); s.adjust = b(8);
    s.uniq = b(9) ? 0.15f : 0.0f;
    s.subpix = b(10) ? SMX_SUBPIX_PARABOLA : 0;
    s.speckle = b(11); s.vote = b(12);
    return s;
}

static void replace_all(std::string& s, const char* from, const char* to) {
    for (size_t at = 0; (at = s.find(from, at)) != std::string::npos; at += strlen(to)) s.replace(at, strlen(from), to);
}

struct Verdict { int rc; PairPlan plan; std::string msg; };

static Verdict plan_of(unsigned key, int cost_mode, int entry) {
    Verdict v;
    char err[512] = "";
    v.rc = plan_pair(settings_of(key, cost_mode), 16, 8, 4, (PairEntry)entry, entry == ENTRY_RGB ? 3 : 0, -3, 0, key >> 14 & 1, key >> 15 & 1,
                     key >> 13 & 1, &v.plan, err, sizeof(err));
    v.msg = err;
    return v;
}

int main() {
    long points = 0, ran = 0, differ = 0, misnamed = 0;
    for (int entry = 0; entry < 3; ++entry)
        for (unsigned key = 0; key < (1u << 16); ++key) {
            const Verdict c = plan_of(key, SMX_COST_CENSUS, entry), m = plan_of(key, SMX_COST_ZNCC, entry);
            ++points;
            ran += m.rc == SMX_OK;
            differ += c.rc != m.rc || memcmp(&c.plan, &m.plan, sizeof(PairPlan)) != 0 ||
                      stages_on(settings_of(key, SMX_COST_CENSUS)) != stages_on(settings_of(key, SMX_COST_ZNCC));
            std::string want = c.msg;
            replace_all(want, "the census cost", "the ZNCC cost");
            replace_all(want, "smx_ctx_set_cost", "smx_ctx_set_zncc");
            misnamed += m.rc != SMX_OK && (m.msg != want || m.msg.find("census") != std::string::npos);
        }
    std::printf("points %ld ran %ld differ %ld misnamed %ld stages %d\n", points, ran, differ, misnamed, (int)N_STAGES);
    std::printf("%s\n", plan_of(1u << 7, SMX_COST_ZNCC, ENTRY_GRAY).msg.c_str());       // PatchMatch stereo
    std::printf("%s\n", plan_of(0, SMX_COST_ZNCC, ENTRY_ASYNC).msg.c_str());            // the pipelined entry
    std::printf("%s\n", plan_of(0, SMX_COST_CENSUS, ENTRY_ASYNC).msg.c_str());        // (the census mode's, unchanged)
    const Verdict plain = plan_of(0, SMX_COST_ZNCC, ENTRY_GRAY), ref = plan_of(0, SMX_COST_REFERENCE, ENTRY_GRAY);
    std::printf("alone: rc %d census %d cost %d; reference: census %d\n", plain.rc, (int)plain.plan.census, (int)plain.plan.cost,
                (int)ref.plan.census);
    return 0;
}
