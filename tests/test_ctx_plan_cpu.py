"""The persistent context's rules -- what a pair runs, needs and refuses under every combination of the opt-in stages -- against
the chain of refusals the context had before it had a stage table (tests/ctx_plan_ref.py), without a GPU.

tests/host_ctx_plan_check.cpp is the stand-alone program (csrc/smx_ctx_plan.h and nothing of the library): it walks the whole
settings space, 2^19 points, and the points this module adds for the pipelined entry and for each per-pair shape limit.  Built
twice with the BUILDS of test_host_twins_cpu.py; the sanitised build is the program itself, nothing preloaded.  For every point
the verdict and every bit of the plan must equal the reference's.  A refused point may name another refusal than the old chain
did where several apply, so the message is held to this: it begins with the entry, and it names by setter only stages that are
on at that point; where exactly one refusal applies it is of that kind and names that refusal's setters.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k ctx_plan
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ctx_plan_ref as ref
from test_host_twins_cpu import BUILDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereo_matching_cuda_amd", "csrc")
ENTRIES = ("smx_ctx_stereo_pair", "smx_ctx_stereo_pair_rgb", "smx_ctx_stereo_pair_async")
KEY_STAGES = ("sgm", "cgf", "cross", "so", "cscale", "perm", "bp", "pm", "adjust", "uniq", "subpix", "speckle", "vote")     # bits 2 ..
SHAPE = dict(w=16, h=8, size_d=4, dminl=-3, dminr=0)
FULL = 2 * (1 << 18)


def key_of(cost=0, mean=False, wants_cost=False, wants_agg=False, **on):
    assert set(on) <= set(KEY_STAGES)
    k = cost | int(mean) << 15 | int(wants_cost) << 16 | int(wants_agg) << 17
    for name in on:
        k |= int(bool(on[name])) << (2 + KEY_STAGES.index(name))
    return k


def settings_of(keys):
    """The settings of ctx_plan_ref.pair from an array of keys."""
    keys = np.asarray(keys, np.int64)
    cost = keys & 3
    s = {name: (keys >> (2 + i) & 1).astype(bool) for i, name in enumerate(KEY_STAGES)}
    s.update(census=cost == 1, adcensus=cost >= 2, adc_colour=cost == 3)
    return s, dict(wants_mean=(keys >> 15 & 1).astype(bool), wants_cost=(keys >> 16 & 1).astype(bool),
                   wants_agg=(keys >> 17 & 1).astype(bool))


def want_bits(need, walker):
    bits = np.zeros(walker.shape, np.int64)
    for i, name in enumerate(ref.NEEDS):
        bits |= need[name].astype(np.int64) << i
    return bits | walker.astype(np.int64) << len(ref.NEEDS)


def extra_points():
    """[(key, entry, channels, w, h, size_d, dminl, dminr)]: the pipelined entry with every single opt-in on and with none, then
    each per-pair shape limit at the limit and just past it."""
    at = (SHAPE["w"], SHAPE["h"], SHAPE["size_d"], SHAPE["dminl"], SHAPE["dminr"])
    pts = [(0, 2, 0) + at] + [(key_of(cost=c), 2, 0) + at for c in (1, 2, 3)] + [(key_of(**{k: True}), 2, 0) + at for k in KEY_STAGES]
    big = 1 << 20
    for stage, lim in (("so", 256), ("bp", 256), ("adjust", 512), ("cscale", big), ("perm", big)):
        pts += [(key_of(**{stage: True}), 0, 0, 16, 8, d, -3, 0) for d in (lim, lim + 1)]
    pts += [(key_of(cgf=True), 1, 3, 16, hh, 4, -3, 0) for hh in (65535, 65536)]
    for dl, dr in ((-big, 0), (-big - 1, 0), (big, big), (0, big + 1), (0, -big), (0, -big - 1)):
        pts.append((key_of(pm=True), 0, 0, 16, 8, 4, dl, dr))
    return pts


@pytest.fixture(scope="module")
def reference():
    """The reference over the whole space and the extra points, computed once."""
    keys = np.tile(np.arange(1 << 18), 2)
    entry = np.repeat([0, 1], 1 << 18)
    out = {"keys": keys, "entry": entry, "full": []}
    for e, ch in ((0, 0), (1, 3)):
        s, wants = settings_of(np.arange(1 << 18))
        out["full"].append(ref.pair(s, channels=ch, **SHAPE, **wants))
    out["extra"] = []
    for key, e, ch, w, h, d, dl, dr in extra_points():
        s, wants = settings_of([key])
        if e == 2:
            out["extra"].append((ref.pair_async(s), {k: np.zeros(1, bool) for k in ref.NEEDS}, np.ones(1, bool)))
        else:
            out["extra"].append(ref.pair(s, w, h, d, ch, dl, dr, **wants))
    return out


def run_program(tmp_path, build):
    exe = str(tmp_path / "host_ctx_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "host_ctx_plan_check.cpp"), "-o", exe])
    work = tmp_path / "out"
    work.mkdir()
    pts = extra_points()
    (work / "extra.txt").write_text("".join(" ".join(str(v) for v in p) + "\n" for p in pts))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    msgs = (work / "messages.txt").read_text().splitlines()
    assert r.stdout == f"points {FULL} extra {len(pts)} messages {len(msgs)}\n"
    table = [l.split("\t") for l in (work / "table.txt").read_text().splitlines()]
    return (np.fromfile(work / "full.i32", "<i4").reshape(-1, 4), np.fromfile(work / "extra.i32", "<i4").reshape(-1, 4), msgs, table)


def ref_names(table):
    """The reference's name of each row of the table, by its setter."""
    by_setter = {v: k for k, v in ref.SETTERS.items()}
    return [by_setter[row[1]] for row in table]


def named_stages(msg, table):
    """The rows whose setter the message names, as a mask (whole names: smx_ctx_set_cross is not smx_ctx_set_cross_scale)."""
    setters = [row[1] for row in table]
    found = re.findall(r"smx_ctx_set_\w+", msg)
    assert all(f in setters for f in found), msg
    return sum(1 << setters.index(f) for f in set(found))


def check_points(got, chains, msgs, table, entries, what):
    """got: the program's records of some points; chains: [(Chain, need, walker)] whose arrays, side by side, cover them."""
    names = ref_names(table)
    refused = np.concatenate([c.refused() for c, _, _ in chains])
    count = np.concatenate([c.count() + np.zeros(c.refused().shape, np.int32) for c, _, _ in chains])
    bits = np.concatenate([want_bits(n, wk) for _, n, wk in chains])
    assert got.shape == (refused.size, 4), (what, got.shape, refused.size)
    rc, plan, mid, on = got.T
    assert set(np.unique(rc).tolist()) <= {0, -1}
    bad = np.flatnonzero((rc != 0) != refused)
    assert bad.size == 0, f"{what}: {bad.size} verdicts differ, first at points {bad[:5]}"
    ok = rc == 0
    bad = np.flatnonzero(ok & (plan != bits))
    assert bad.size == 0, f"{what}: {bad.size} plans differ, first at points {bad[:5]}: {plan[bad[:5]]} != {bits[bad[:5]]}"
    assert (mid[ok] == -1).all() and (mid[~ok] >= 0).all() and mid.max() < len(msgs)
    # every message begins with its entry and names only stages that are on
    named = np.array([named_stages(m, table) for m in msgs], np.int64)
    starts = np.array([[m.startswith(e + ": ") for m in msgs] for e in ENTRIES])
    r = np.flatnonzero(~ok)
    assert starts[entries[r], mid[r]].all(), what
    assert (named[mid[r]] != 0).all() and (named[mid[r]] & ~on[r].astype(np.int64) == 0).all(), what
    # exactly one refusal applies: it is that one
    at = 0
    checked = 0
    for c, _, _ in chains:
        n = c.refused().size
        sl = slice(at, at + n)
        single = count[sl] == 1
        for cond, kind, stages in c.refusals:
            here = np.flatnonzero(cond & single) + at
            if here.size == 0:
                continue
            want_named = sum(1 << names.index(s) for s in stages)
            for i in np.unique(mid[here]):
                m = msgs[i]
                assert named[i] == want_named, (what, kind, stages, m)
                if kind == "conflict":
                    assert "do not run together" in m and all(table[names.index(s)][5] in m for s in stages), m
                elif kind == "mean":
                    assert "produces no mean images" in m and table[names.index(stages[0])][5] in m, m
                elif kind == "shape":
                    assert table[names.index(stages[0])][6] and table[names.index(stages[0])][6] in m, m
                elif kind == "entry":
                    assert "use smx_ctx_stereo_pair_rgb" in m, m
                elif kind == "pm_out":
                    assert "produces no" in m, m
                else:
                    assert kind == "async" and table[names.index(stages[0])][5] + " is on" in m and m.endswith("use " + ref.ASYNC_USE[stages[0]]), m
            checked += here.size
        at += n
    assert checked == int((count == 1).sum()), what
    return on


def design_matrix(table):
    """The stage table as the markdown table of DESIGN.md §4.3r: a row per stage; x where two stages do not run together."""
    names = ref_names(table)
    head = ["stage (setter)"] + names + ["mean images", "shape limit", "checked"]
    lines = ["| " + " | ".join(head) + " |", "|" + "---|" * len(head)]
    for i, row in enumerate(table):
        excl, checked = int(row[2]), int(row[4])
        cells = ["-" if i == j else "x" if excl >> j & 1 else "" for j in range(len(table))]
        where = {0: "", 1: "setter", 2: "pair", 3: "setter, pair"}[checked]
        lines.append("| " + " | ".join([f"{row[5]} (`{row[1]}`)"] + cells + ["no" if row[3] == "1" else "", row[6][6:].replace("|", "\\|") if checked else "",
                                        where]) + " |")
    return lines


@pytest.mark.parametrize("build", list(BUILDS))
def test_every_point_plans_and_refuses_as_the_old_chain_did(tmp_path, reference, build):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    full, extra, msgs, table = run_program(tmp_path, build)
    names = ref_names(table)
    assert len(table) == 15 and sorted(names) == sorted(ref.SETTERS) and [int(r[0]) for r in table] == list(range(15))
    # no point is left out
    assert full.shape == (FULL, 4) and extra.shape == (len(extra_points()), 4)
    on = check_points(full, reference["full"], msgs, table, reference["entry"], build + " full")
    # stages_on() reads the settings as the reference names them
    s, _ = settings_of(reference["keys"])
    want_on = sum(s[name].astype(np.int64) << i for i, name in enumerate(names))
    assert np.array_equal(on, want_on)
    assert 0 < int((full[:, 0] == 0).sum()) < FULL // 8                         # (most combinations are refused)
    pts = extra_points()
    for i, p in enumerate(pts):
        check_points(extra[i:i + 1], [reference["extra"][i]], msgs, table, np.array([p[1]]), f"{build} extra point {p}")
    # the points at a limit pass, the points just past it do not, and the pipelined entry takes the all-off state only
    verdicts = extra[:, 0].tolist()
    assert verdicts[:17] == [0] + [-1] * 16
    assert verdicts[17:29] == [0, -1] * 6 and verdicts[29:] == [0, -1, 0, -1, 0, -1]
    # the table's conflicts: each listed pair is refused with only those two on, whichever of the two the message names first,
    # and the table lists a pair from both sides
    excl = [int(r[2]) for r in table]

    def both_on(a, b):
        """The key with rows a and b on and nothing else (census and AD-Census are two values of one setting: never both)."""
        cost = {"census": 1, "adcensus": 2}
        assert {names[a], names[b]} != set(cost)
        return key_of(cost=max(cost.get(names[a], 0), cost.get(names[b], 0)), **{n: True for n in (names[a], names[b]) if n in KEY_STAGES})

    listed = 0
    for a in range(15):
        for b in range(15):
            assert (excl[a] >> b & 1) == (excl[b] >> a & 1) and not excl[a] >> a & 1
            if a >= b or {names[a], names[b]} == {"census", "adcensus"}:
                continue
            for e in (0, 1):
                rec = full[e * (1 << 18) + both_on(a, b)]
                if not excl[a] >> b & 1:
                    # what the table does not list runs (on the rgb entry, which takes colour guidance)
                    assert e == 0 or rec[0] == 0, (names[a], names[b])
                    continue
                assert rec[0] == -1, (names[a], names[b])
                m = msgs[rec[2]]
                assert m.startswith(ENTRIES[e]) and "do not run together" in m and table[a][1] in m and table[b][1] in m, m
                assert named_stages(m, table) == (1 << a | 1 << b), m
            listed += excl[a] >> b & 1
    # (3 guided-only x 5 replacing, 10 pairs of replacing less cross + scan-line, permeability + cross-scale, 5 more of PatchMatch)
    assert listed == 15 + 9 + 1 + 5

def test_design_md_shows_the_table_as_the_header_has_it(tmp_path):
    """The conflict matrix of DESIGN.md §4.3r is design_matrix() of the table the program prints, line for line."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    table = run_program(tmp_path, "plain")[3]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert "\n".join(design_matrix(table)) + "\n" in text
