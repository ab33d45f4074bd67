"""CPU-side lint of the comb walker's hand-off from its gfx950 ISA (hipcc cross-compiles; no GPU): the counted wait behind the
record store, the release of tile 2, the sc1 bits (tools/v5_handoff_check.py).  Every rule is shown a few lines of hand-written
assembly that it has to pass and to fail, then all rules run on the real builds (one compile each, kept by tools/v5_asm.sh and
shared with tests/test_isa_lint.py)."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("v5_handoff_check", os.path.join(ROOT, "tools", "v5_handoff_check.py"))
lint = importlib.util.module_from_spec(spec)
spec.loader.exec_module(lint)

REC = "buffer_store_dwordx4 v[6:9], v11, s[88:91], 0 offen sc1"
Q = "buffer_store_dword v8, v111, s[12:15], s10 offen nt"
GUID = ["buffer_load_dwordx4 v[6:9], v6, s[84:87], s11 offen", "buffer_load_dword v114, v112, s[84:87], s10 offen"]


def mark(name):
    return [";;#ASMSTART", "; MARK " + name, ";;#ASMEND"]


def hand(ins):
    return [";;#ASMSTART", ins, ";;#ASMEND"]


def head(reads=("ds_read2st64_b32 v[88:89], v7 offset0:6 offset1:9",), wait=("s_waitcnt lgkmcnt(0)",), add=("ds_add_u32 v107, v106",),
         after=(), rec=(REC,)):
    """the slot's head as the compiler lays it out: the band out of tile 2, the wait, the release, the record under its condition"""
    return (mark("s2head begin") + list(reads) + list(wait) + ["s_and_saveexec_b64 s[44:45], s[6:7]"] + list(add) + list(after)
            + ["s_or_b64 exec, exec, s[44:45]", "s_and_saveexec_b64 s[44:45], s[42:43]", "s_cbranch_execz .LBB0_1"] + list(rec)
            + [".LBB0_1:", "s_or_b64 exec, exec, s[44:45]"] + mark("s2head end"))


def site(n, rows=(Q, Q), border=(Q, Q, Q, Q, Q), behind_head=(), head_lines=None):
    """one stage-2 slot: head, then no rows (sl < 2) / border rows / marked interior rows, the guidance loads, drain or counted wait"""
    return ((head() if head_lines is None else head_lines) + list(behind_head)
            + ["s_cbranch_scc1 .LBB0_4", "s_cbranch_vccnz .LBB0_3"] + mark("s2rows begin") + list(rows) + mark("s2rows end")
            + ["s_branch .LBB0_4", ".LBB0_3:"] + list(border)
            + [".LBB0_4:"] + GUID + ["s_cbranch_vccz .LBB0_5"] + hand("s_waitcnt vmcnt(0)") + ["s_branch .LBB0_6", ".LBB0_5:"]
            + hand(f"s_waitcnt vmcnt({n})") + [".LBB0_6:", "s_barrier"])


def func(lines, name="frag"):
    return lint.parse(list(lines) + ["s_endpgm"], fragment=name)[0]


def rules(findings):
    return sorted({x.rule for x in findings})


def test_the_parser_builds_functions_blocks_and_edges():
    text = ["\t.text", "_Z1fv:                                  ; @_Z1fv", "; %bb.0:", "\ts_cbranch_scc1 .LBB0_2", "; %bb.1:", "\ts_branch .LBB0_3",
            ".LBB0_2:                                ; %x", "\tv_mov_b32_e32 v0, 0", ".LBB0_3:", "\ts_endpgm", ".Lfunc_end0:", "\t.size _Z1fv, .Lfunc_end0-_Z1fv",
            "_Z1gv:                                  ; @_Z1gv", "\ts_endpgm", ".Lfunc_end1:"]
    f, g = lint.parse(text)
    assert (f.name, g.name) == ("_Z1fv", "_Z1gv")
    assert [x.op for x in f.ins] == ["s_cbranch_scc1", "s_branch", "v_mov_b32_e32", "s_endpgm"] and [x.line for x in f.ins] == [4, 6, 8, 10]
    assert f.succ == [[2, 1], [3], [3], []] and f.pred[3] == [1, 2] and not f.broken
    h = func(hand("s_waitcnt vmcnt(3)") + ["s_waitcnt vmcnt(2) lgkmcnt(0)", "s_waitcnt 0x0070"])
    assert [x.hand for x in h.ins] == [True, False, False, False]
    assert lint.waits(h.ins[1]) == {"vmcnt": 2, "lgkmcnt": 0} and lint.waits(h.ins[2]) == {"vmcnt": 0, "expcnt": 7, "lgkmcnt": 0}


def test_r1_the_counted_wait_covers_the_record():
    ok, notes = lint.r1(func(site(4)))                          # two rows + two loads behind the record store
    assert ok == [] and len(notes) == 1 and "N = 4, counted minimum 4" in notes[0] and "more" not in notes[0]
    ok, notes = lint.r1(func(site(3)))                          # waits for more than the record: safe, a note
    assert ok == [] and "counted minimum 4" in notes[0] and "waits for more than the record" in notes[0]
    bad, notes = lint.r1(func(site(5)))                         # the text from the record store to the wait holds 9: the graph gives 4
    assert rules(bad) == ["R1"] and notes == [] and "issues only 4" in bad[0].msg and bad[0].func == "frag"
    assert bad[0].line == func(site(5)).ins[lint.counted_waits(func(site(5)))[0]].line
    # a diamond in the rows whose other arm holds more stores: the minimum goes through the poorer arm
    diamond = [Q, "s_cbranch_vccz .LBB0_10", Q, Q, Q, "s_branch .LBB0_11", ".LBB0_10:", Q, ".LBB0_11:"]
    assert lint.r1(func(site(4, rows=diamond)))[0] == []
    assert rules(lint.r1(func(site(5, rows=diamond)))[0]) == ["R1"]
    # a store in a conditionally skipped block does not count
    skipped = [Q, "s_and_saveexec_b64 s[10:11], vcc", "s_cbranch_execz .LBB0_10", Q, ".LBB0_10:", "s_or_b64 exec, exec, s[10:11]"]
    assert lint.r1(func(site(3, rows=skipped)))[0] == []
    assert "issues only 3" in lint.r1(func(site(4, rows=skipped)))[0][0].msg
    # a loop: the back-edge gives one trip of a bottom-tested loop, none of a top-tested one, whatever the trip count
    loop = [".LBB0_10:", "global_atomic_add_u32 v1, v2, s[2:3]", Q, "s_cbranch_scc1 .LBB0_10"]
    assert lint.r1(func(site(4, rows=loop)))[0] == []
    assert "issues only 4" in lint.r1(func(site(5, rows=loop)))[0][0].msg
    top = [".LBB0_10:", "s_cbranch_scc0 .LBB0_11", Q, Q, "s_branch .LBB0_10", ".LBB0_11:"]
    assert lint.r1(func(site(2, rows=top)))[0] == []
    assert "issues only 2" in lint.r1(func(site(3, rows=top)))[0][0].msg
    # flat_* and LDS instructions are not counted, cache maintenance is left out
    assert "issues only 3" in lint.r1(func(site(4, rows=[Q, "flat_store_dword v[2:3], v1", "ds_write_b32 v1, v2", "buffer_wbl2 sc1"])))[0][0].msg


def test_r1_is_anchored_at_the_marks_and_the_record_store():
    assert "holds 0 16-byte sc1" in lint.r1(func(site(4, head_lines=head(rec=[REC.replace(" sc1", "")]))))[0][0].msg
    assert "holds 2 16-byte sc1" in lint.r1(func(site(4, head_lines=head(rec=[REC, REC]))))[0][0].msg
    assert "holds 0 16-byte sc1" in lint.r1(func(site(4, head_lines=head(rec=[REC.replace("dwordx4 v[6:9]", "dwordx2 v[6:7]")]))))[0][0].msg
    bad = lint.r1(func(site(4, behind_head=[REC])))[0]          # a second record store behind the head: the count starts in front of it
    assert rules(bad) == ["R1"] and "between `s2head end`" in bad[0].msg
    assert "between `s2head end`" in lint.r1(func(site(4, border=[Q, REC])))[0][0].msg
    # the wait without a rows mark in front of it, and with two
    lines = site(4)
    i = lines.index("; MARK s2rows begin")
    assert "reached from 0 `s2rows begin`" in lint.r1(func(lines[:i - 1] + lines[i + 2:]))[0][0].msg
    two = site(4, border=mark("s2rows begin") + [Q, Q])
    assert "reached from 2 `s2rows begin`" in lint.r1(func(two))[0][0].msg
    # rows without a head in front of them
    i = lines.index("; MARK s2head end")
    assert "not led to by exactly one `s2head` region" in lint.r1(func(lines[i + 2:]))[0][0].msg
    # a second slot behind the first: each wait belongs to its own rows mark
    second = [l.replace(".LBB0_", ".LBB1_") for l in site(6, rows=[Q] * 4)]
    ok, notes = lint.r1(func(site(4) + second))
    assert ok == [] and len(notes) == 2 and "N = 6, counted minimum 6" in notes[1]
    assert len(lint.r1(func(site(5) + second))[0]) == 1
    # a branch that leaves the graph
    assert "leaves the function's graph" in lint.r1(func(site(4, rows=[Q, Q, "s_setpc_b64 s[30:31]"])))[0][0].msg
    assert "leaves the function's graph" in lint.r1(func(site(4, rows=[Q, Q, "s_cbranch_scc1 .LBB7_1"])))[0][0].msg
    # the compiler's own counted waits are no sites
    assert lint.counted_waits(func(["s_waitcnt vmcnt(3)"] + hand("s_waitcnt vmcnt(0)"))) == []


def test_r2_is_not_vacuous(tmp_path):
    assert lint.r2(func(site(4)), 4) == []
    assert "N = [4], the source's constants give 5" in lint.r2(func(site(4)), 5)[0].msg
    both = site(4) + [l.replace(".LBB0_", ".LBB1_") for l in site(6, rows=[Q] * 4)]
    assert "N = [4, 6]" in lint.r2(func(both), 4)[0].msg
    lines = site(4)
    i = lines.index("s_waitcnt vmcnt(4)")
    assert "no hand-written counted wait" in lint.r2(func(lines[:i - 1] + lines[i + 2:]), 4)[0].msg
    assert "no hand-written counted wait" in lint.r2(func(lines[:i - 1] + ["s_waitcnt vmcnt(4)"] + lines[i + 2:]), 4)[0].msg
    msgs = " ".join(x.msg for x in lint.r2(func(hand("s_waitcnt vmcnt(4)")), 4))
    for what in ("`s2rows begin` mark", "`s2head begin` mark", "vector-memory instruction", "ds_* instruction"):
        assert f"no {what}" in msgs
    out, notes = lint.check_marked(lint.parse(["_Z5otherv:     ; @_Z5otherv", "s_endpgm", ".Lfunc_end0:"]))
    assert rules(out) == ["R2"] and "no k_v5_walk function" in out[0].msg
    # the expected N come from the source's constants
    (tmp_path / "smx_agg_v5.hip").write_text("constexpr int S2_KEEP = 14;     // ...\n")
    (tmp_path / "smx_agg_v5.h").write_text("constexpr int BH = 6;                  // band height\n")
    assert (lint.expected_keep(0, str(tmp_path)), lint.expected_keep(1, str(tmp_path))) == (14, 11)
    walker = ["_ZN3smx2v59k_v5_walkILi0ELi1EEEvNS0_4ArgsE: ; @_ZN3smx2v59k_v5_walkILi0ELi1EEEvNS0_4ArgsE"]
    real = site(11, rows=[Q] * 9, head_lines=head() + ["buffer_load_dwordx4 v[2:5], v1, s[88:91], 0 offen sc1"])
    assert lint.check_marked(lint.parse(walker + real + ["s_endpgm", ".Lfunc_end0:"]), str(tmp_path))[0] == []
    out = lint.check_marked(lint.parse([walker[0].replace("Li1EEE", "Li0EEE")] + real + ["s_endpgm", ".Lfunc_end0:"]), str(tmp_path))[0]
    assert rules(out) == ["R2"] and "give 14" in out[0].msg


def test_r3_the_ordering_premise():
    assert lint.r3(func(site(4))) == []
    assert [x.rule for x in lint.r3(func(site(4, rows=[Q, "flat_load_dword v1, v[2:3]", Q])))] == ["R3"]
    assert [x.rule for x in lint.r3(func(["scratch_load_dword v1, off, s0"] + site(4)))] == ["R3"]


def test_r4_tile_2_is_released_after_it_was_read():
    rd = "ds_read_b32 v6, v7"
    assert lint.r4(func(site(4))) == []
    assert lint.r4(func(site(4, head_lines=head(wait=["s_waitcnt vmcnt(1) lgkmcnt(0)"])))) == []
    assert lint.r4(func(site(4, head_lines=head(wait=["s_waitcnt 0x0070"])))) == []
    for wait in ([], ["s_waitcnt lgkmcnt(1)"], ["s_waitcnt vmcnt(0)"], ["s_waitcnt lgkmcnt(0)", rd]):
        bad = lint.r4(func(site(4, head_lines=head(wait=wait))))
        assert rules(bad) == ["R4"] and "no `s_waitcnt lgkmcnt(0)` lies behind the last ds_read*" in bad[0].msg
    # the wait moved behind the add
    assert "no `s_waitcnt lgkmcnt(0)`" in lint.r4(func(site(4, head_lines=head(wait=[], after=["s_waitcnt lgkmcnt(0)"]))))[0].msg
    # a read on one arm only, behind the wait of the other
    arm = ["s_waitcnt lgkmcnt(0)", "s_cbranch_execz .LBB0_20", rd, ".LBB0_20:"]
    assert "no `s_waitcnt lgkmcnt(0)`" in lint.r4(func(site(4, head_lines=head(wait=arm))))[0].msg
    assert lint.r4(func(site(4, head_lines=head(wait=arm + ["s_waitcnt lgkmcnt(0)"])))) == []
    # a wait on one arm only
    arm = ["s_cbranch_execz .LBB0_20", "s_waitcnt lgkmcnt(0)", ".LBB0_20:"]
    assert "no `s_waitcnt lgkmcnt(0)`" in lint.r4(func(site(4, head_lines=head(wait=arm))))[0].msg
    # a read behind the release, one add exactly
    assert "reads LDS behind the ds_add_u32" in lint.r4(func(site(4, head_lines=head(after=[rd]))))[0].msg
    assert "reads LDS behind the ds_add_u32" in lint.r4(func(site(4, head_lines=head(rec=[rd, REC]))))[0].msg
    assert lint.r4(func(site(4, behind_head=[rd]))) == []        # behind `s2head end` the tile is stage 1's business
    assert "holds 0 ds_add_u32" in lint.r4(func(site(4, head_lines=head(add=[]))))[0].msg
    assert "holds 2 ds_add_u32" in lint.r4(func(site(4, head_lines=head(add=["ds_add_u32 v107, v106"] * 2))))[0].msg
    lines = site(4)
    i = lines.index("; MARK s2head end")
    assert "reaches 0 `s2head end`" in lint.r4(func(lines[:i - 1] + lines[i + 2:]))[0].msg


def test_r5_hand_off_accesses_are_sc1():
    hand_in = "buffer_load_dwordx4 v[2:5], v1, s[88:91], 0 offen sc1"
    assert lint.r5(func([hand_in] + site(4))) == []
    bad = lint.r5(func(site(4)))
    assert rules(bad) == ["R5"] and "hand-in load has lost its sc1" in bad[0].msg
    bad = lint.r5(func([hand_in.replace(" sc1", "")] + site(4)))
    assert len(bad) == 2 and "uses the descriptor s[88:91] of a record store without sc1" in bad[0].msg
    bad = lint.r5(func([hand_in, "buffer_load_dword v1, v2, s[88:91], 0 offen"] + site(4)))
    assert len(bad) == 1 and "reused the SGPR quad" in bad[0].msg
    assert lint.r5(func([hand_in, "buffer_load_dword v1, v2, s[84:87], 0 offen", "buffer_load_dword v1, v2, s[88:91], 0 offen sc1 nt"] + site(4))) == []
    bad = lint.r5(func([hand_in] + site(4, head_lines=head(rec=[REC.replace(" sc1", "")]))))
    assert len(bad) == 1 and "record stores have lost their sc1" in bad[0].msg


def test_r6_the_product_build_matches_the_marked_build():
    hand_in = "buffer_load_dwordx4 v[2:5], v1, s[88:91], 0 offen sc1"
    strip = lambda lines: [l for l in lines if "MARK" not in l]
    m = [func([hand_in] + site(4), "f")]
    assert lint.r6_functions(m, [func(strip([hand_in] + site(4, rows=["v_mov_b32_e32 v1, v2", Q, "s_nop 0", Q])), "f")]) == []
    for other, what in ((site(4, rows=[Q]), "buffer_store_dword: 7 in the marked build, 6"), (site(5), "hand-written s_waitcnt vmcnt(4): 1 in the marked build, 0"),
                        (site(4) + ["s_barrier"], "s_barrier: 1 in the marked build, 2"), (site(4, head_lines=head(add=[])), "ds_add_u32: 1 in the marked build, 0"),
                        (site(4, rows=[Q, Q.replace("dword ", "dwordx2 ")]), "buffer_store_dwordx2: 0 in the marked build, 1")):
        bad = lint.r6_functions(m, [func(strip([hand_in] + other), "f")])
        assert rules(bad) == ["R6"] and any(what in x.msg for x in bad), (what, bad)
    assert "the product build has no such function" in lint.r6_functions(m, [])[0].msg
    assert "the marked build has no such function" in lint.r6_functions([], m)[0].msg
    assert rules(lint.r6_functions(m, [func(strip([hand_in, "flat_load_dword v1, v[2:3]"] + site(4)), "f")])) == ["R6/R3"]
    assert rules(lint.r6_functions([func(site(4), "f")], [func(strip(site(4)), "f")])) == ["R6/R5"]


def test_r6_the_flags_are_read_from_both_files():
    mk = "HIPCC ?= hipcc\nCXXFLAGS = -O3 -std=c++17 --offload-arch=$(ARCH) -ffp-contract=off \\\n    -mllvm -x=None -I$(ROOT)/include -Wall -Wno-unused-function $(EXTRA)\nSRCS = a.hip\n"
    sh = ("set -e\n/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off \\\n  -mllvm -x=None $MARK \"$@\" -I$ROOT/include \\\n"
          "  --save-temps -c $ROOT/csrc/a.hip -o x.o >/dev/null 2>&1\ncp a.s $OUT\n")
    assert lint.r6_flags(sh, mk) == []
    assert lint.r6_flags(sh.replace("$MARK", "-DSMX_V5_MARK"), mk) == []
    assert "only in the script ['-ffast-math']" in lint.r6_flags(sh.replace("-mllvm", "-ffast-math -mllvm"), mk)[0].msg
    assert "only in the Makefile ['-ffp-contract=off']" in lint.r6_flags(sh.replace("-ffp-contract=off ", ""), mk)[0].msg
    assert "only in the script ['-O3'], only in the Makefile ['-O2']" in lint.r6_flags(sh, mk.replace("-O3", "-O2"))[0].msg
    assert "only in the script ['-DX=1']" in lint.r6_flags(sh.replace("$MARK", "$MARK -DX=1"), mk)[0].msg
    assert "could not be read" in lint.r6_flags("echo nothing\n", mk)[0].msg
    assert "could not be read" in lint.r6_flags(sh, "all:\n")[0].msg


def test_r7_one_counted_wait_in_the_source():
    keep = 'constexpr int KEEP = QPERM ? S2_KEEP - BH / 2 : S2_KEEP;\nif (s2_interior) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(KEEP) : "memory"); else\ndrain_vmem();\n'
    drain = '__device__ void drain_vmem() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }\n// vmcnt(3) in a comment\n'
    assert lint.r7({"csrc/smx_agg_v5.hip": keep, "csrc/smx_agg_dev.h": drain}) == []
    bad = lint.r7({"csrc/smx_agg_v5.hip": keep + '\n\nasm volatile("s_waitcnt vmcnt(3)" ::: "memory");\n', "csrc/smx_agg_dev.h": drain})
    assert rules(bad) == ["R7"] and bad[0].line == 6 and "vmcnt(3)" in bad[0].msg
    assert "vmcnt(2)" in lint.r7({"csrc/smx_agg_v5.hip": keep, "csrc/smx_agg_v4.hip": 'asm volatile("s_nop 0\\n\\ts_waitcnt vmcnt(2) lgkmcnt(0)");'})[0].msg
    assert "vmcnt(%0)" in lint.r7({"csrc/smx_agg_v5.hip": keep, "csrc/smx_agg_v4.hip": keep})[0].msg
    assert "vmcnt(%0)" in lint.r7({"csrc/smx_agg_v5.hip": keep + 'asm volatile("s_waitcnt vmcnt(%0)" :: "n"(OTHER));'})[0].msg
    assert "vmcnt(1)" in lint.r7({"csrc/smx_agg_v5.hip": keep + '__asm__ volatile("s_waitcnt vmcnt(1)");'})[0].msg
    assert "the KEEP site was not found" in lint.r7({"csrc/smx_agg_v5.hip": drain})[0].msg


def test_comb_walker_hand_off_holds_on_the_marked_and_the_product_build(capsys):
    assert lint.main([]) == 0
    out = capsys.readouterr().out
    sites = re.findall(r"k_v5_walkILi\dELi(\d)E\S*: vmcnt\((\d+)\) at line \d+: N = (\d+), counted minimum (\d+)", out)
    assert len({l.split(":")[0] for l in out.split("\n") if "counted minimum" in l}) == 4, out      # the four instantiations of the launch
    assert all(int(n) == lint.expected_keep(int(qp)) and int(k) >= int(n) for qp, n, _, k in sites) and len(sites) >= 4
