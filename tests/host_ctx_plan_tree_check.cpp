// The tree filter in the persistent context's rules (stereo_matching_cuda_amd/csrc/smx_ctx_plan.h): a second mode of the
// permeability filter's row of the stage table under its own name.  A stand-alone program, built and run by
// tests/test_ctx_plan_tree_cpu.py on the CPU only -- once plain, once under -fsanitize=address,undefined.
//
//   host_ctx_plan_tree_check
//
// It walks every combination of the fourteen other stages (bits 0-13: SGM, colour guidance, cross, scan-line, cross-scale, bp,
// PatchMatch, adjust, uniqueness, sub-pixel, speckle, vote, the census cost, AD-Census) and of the wanted outputs (bits 14-16:
// mean images, cost volumes, aggregated volumes) on the three entries, once with the permeability filter on and once with the
// tree filter on, and counts the points where the two differ in the verdict, in any bit of the plan or in stages_on(), and the
// refused points whose message is not the permeability mode's with the noun and the setter replaced.  Then it prints the
// messages of four refusals and what the row plans alone.
#include <cstdio>
#include <cstring>
#include <string>

#include "smx_ctx_plan.h"

using namespace smx;

enum Mode { OFF, PERM, TREE };

static CtxSettings settings_of(unsigned key, Mode mode) {
    CtxSettings s;
    auto b = [key](int i) { return (key >> i & 1) != 0; };
    s.agg_mode = b(0) ? SMX_AGG_SGM : SMX_AGG_GUIDED;
    s.guide_mode = b(1) ? SMX_GUIDE_RGB : SMX_GUIDE_GRAY;
    s.cross = b(2); s.so = b(3); s.cscale = b(4); s.bp = b(5); s.pm = b(6); s.adjust = b(7);
    s.uniq = b(8) ? 0.15f : 0.0f;
    s.subpix = b(9) ? SMX_SUBPIX_PARABOLA : 0;
    s.speckle = b(10); s.vote = b(11);
    s.cost_mode = b(12) ? SMX_COST_CENSUS : SMX_COST_REFERENCE;
    s.adcensus = b(13);
    s.perm = mode == PERM;
    s.tree = mode == TREE;
    return s;
}

static void replace_all(std::string& s, const char* from, const char* to) {
    for (size_t at = 0; (at = s.find(from, at)) != std::string::npos; at += strlen(to)) s.replace(at, strlen(from), to);
}

struct Verdict { int rc; PairPlan plan; std::string msg; };

static Verdict plan_of(unsigned key, Mode mode, int entry) {
    Verdict v;
    char err[512] = "";
    v.rc = plan_pair(settings_of(key, mode), 16, 8, 4, (PairEntry)entry, entry == ENTRY_RGB ? 3 : 0, -3, 0, key >> 15 & 1, key >> 16 & 1,
                     key >> 14 & 1, &v.plan, err, sizeof(err));
    v.msg = err;
    return v;
}

int main() {
    long points = 0, ran = 0, differ = 0, misnamed = 0;
    for (int entry = 0; entry < 3; ++entry)
        for (unsigned key = 0; key < (1u << 17); ++key) {
            const Verdict p = plan_of(key, PERM, entry), t = plan_of(key, TREE, entry);
            ++points;
            ran += t.rc == SMX_OK;
            differ += p.rc != t.rc || memcmp(&p.plan, &t.plan, sizeof(PairPlan)) != 0 ||
                      stages_on(settings_of(key, PERM)) != stages_on(settings_of(key, TREE));
            std::string want = p.msg;
            replace_all(want, "the permeability filter", "the tree filter");
            replace_all(want, "smx_ctx_set_permeability", "smx_ctx_set_tree");
            misnamed += t.rc != SMX_OK && (t.msg != want || t.msg.find("permeability") != std::string::npos);
        }
    std::printf("points %ld ran %ld differ %ld misnamed %ld stages %d\n", points, ran, differ, misnamed, (int)N_STAGES);
    std::printf("%s\n", plan_of(1u << 0, TREE, ENTRY_GRAY).msg.c_str());        // semi-global matching
    std::printf("%s\n", plan_of(1u << 4, TREE, ENTRY_GRAY).msg.c_str());        // cross-scale aggregation
    std::printf("%s\n", plan_of(0, TREE, ENTRY_ASYNC).msg.c_str());             // the pipelined entry
    std::printf("%s\n", plan_of(0, PERM, ENTRY_ASYNC).msg.c_str());             // (the permeability mode's, unchanged)
    std::printf("%s\n", plan_of(1u << 14, TREE, ENTRY_GRAY).msg.c_str());       // mean images
    const Verdict alone = plan_of(0, TREE, ENTRY_GRAY), off = plan_of(0, OFF, ENTRY_GRAY);
    std::printf("alone: rc %d perm %d agg %d cost %d walker %d; off: perm %d agg %d\n", alone.rc, (int)alone.plan.perm, (int)alone.plan.agg,
                (int)alone.plan.cost, (int)alone.plan.walker_status, (int)off.plan.perm, (int)off.plan.agg);
    // the setters' mutual refusal (the rule they call), and that neither mode stands in its own way or in the way of switching off
    auto text = [](const char* s) { return s ? s : "-"; };
    std::printf("%s\n", text(row_mode_conflict(settings_of(0, PERM), true)));
    std::printf("%s\n", text(row_mode_conflict(settings_of(0, TREE), false)));
    std::printf("%s %s %s %s\n", text(row_mode_conflict(settings_of(0, TREE), true)), text(row_mode_conflict(settings_of(0, PERM), false)),
                text(row_mode_conflict(settings_of(0, OFF), true)), text(row_mode_conflict(settings_of(0, OFF), false)));
    return 0;
}
