"""The CPU twin of region voting (host/cpu_twins.cpp: region_voteOnCPU) against tests/vote_ref.py, bit for bit, without a GPU
-- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --vote --host-compare` trusts.  tests/host_vote_check.cpp is the stand-alone program that runs it (no
libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files and writes the twin's output
beside them; the comparison with the values of vote_ref is made here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_vote
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import vote_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

# w, h, channels, D, dmin, d_lr, tau_s, tau_h_pct, iterations, interpolate, l1, l2, tau1, tau2, have_right, guide, map: one pixel,
# one row, one column, every channel count, the longest arm, every number of rounds at the ends of its range, both forms of the
# interpolation, messy maps, d_lr 0 and 1
CASES = [(1, 1, 1, 1, 0, 0, 20, 40, 5, 1, 34, 17, 20, 6, 1, "constant", "plain"),
         (40, 1, 3, 3, -2, 0, 2, 40, 2, 1, 17, 8, 20, 6, 1, "textured", "plain"),
         (1, 23, 4, 2, 0, 1, 0, 0, 8, 1, 63, 0, 20, 6, 0, "constant", "messy"),
         (33, 21, 3, 4, -3, 1, 5, 30, 1, 1, 63, 63, 30, 30, 1, "constant", "messy"),
         (64, 24, 3, 8, -4, 0, 20, 40, 5, 1, 9, 4, 20, 6, 1, "textured", "plain"),
         (31, 17, 1, 5, 0, 0, 3, 99, 3, 0, 5, 0, 256, 256, 1, "checkerboard", "messy"),
         (20, 30, 4, 16, 1, 2, 1, 10, 0, 1, 34, 17, 12, 1, 1, "textured", "messy"),
         (45, 19, 1, 6, -8, 0, 0, 0, 4, 1, 4, 2, 256, 256, 0, "checkerboard", "plain")]


def _case(k, w, h, ch, D, dmin, d_lr, tau_s, pct, it, interp, l1, l2, tau1, tau2, have_right, guide, kind):
    g, d, dr = ref.scene(60 + k, h, w, dmin, D, guide, kind, ch)
    want = ref.region_vote_guide(d, g, dr if have_right else None, dmin, D, d_lr, cross=dict(l1=l1, l2=l2, tau1=tau1, tau2=tau2),
                                 tau_s=tau_s, tau_h_pct=pct, iterations=it, interpolate_=interp)
    stem = f"case{k}"
    inputs = {"guide.u8": g, "disp.f32": d}
    if have_right:
        inputs["right.f32"] = dr
    return {"line": f"vote {stem} {w} {h} {ch} {D} {dmin} {d_lr} {tau_s} {pct} {it} {interp} {l1} {l2} {tau1} {tau2} {have_right}",
            "stem": stem, "want": want, "inputs": inputs, "changed": int((want.view(np.uint32) != d.view(np.uint32)).sum())}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = [_case(k, *c) for k, c in enumerate(CASES)]
    assert sum(c["changed"] > 0 for c in cs) >= 6           # the cases do something
    exe = str(tmp_path / "host_vote_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_vote_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(c["line"] for c in cs) + "\n")
    for c in cs:
        for suffix, a in c["inputs"].items():
            a = np.ascontiguousarray(a)
            a.astype(a.dtype.newbyteorder("<")).tofile(work / f"{c['stem']}.{suffix}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(cs)}\n" in r.stdout
    for c in cs:
        got = np.fromfile(work / f"{c['stem']}.voted.f32", "<f4").reshape(c["want"].shape)
        same = got.view(np.uint32) == c["want"].view(np.uint32)
        assert same.all(), f"{c['line']}: {(~same).sum()} of {same.size} elements differ"
