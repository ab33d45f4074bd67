"""The CPU twin of the cross-based aggregation (host/cpu_twins.cpp: cross_aggregateOnCPU) against tests/cross_ref.py, bit for
bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --aggregation cross --host-compare` trusts.  tests/host_cross_check.cpp is the stand-alone program
that runs it (no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files and writes
the twin's outputs beside them; the comparison with the values of cross_ref is made here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_cross
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx

import cross_ref as ref
from test_cross_cpu import textured_guide
from test_host_twins_cpu import BUILDS, HOST, ROOT

# w, h, channels, D, dmin, l1, l2, tau1, tau2, iterations, want_agg: one pixel, one row, one column, every channel count, the
# longest arm on an image smaller than it, open thresholds, l2 = 0 and l2 = l1, every number of iterations
CASES = [(1, 1, 1, 1, 0, 34, 17, 20, 6, 4, 1), (40, 1, 3, 3, -2, 17, 8, 20, 6, 2, 1), (1, 23, 4, 2, 0, 63, 0, 20, 6, 3, 0),
         (33, 21, 3, 4, -3, 63, 63, 30, 30, 1, 1), (64, 24, 3, 5, -4, 9, 4, 20, 6, 4, 1), (31, 17, 1, 2, 0, 5, 0, 256, 256, 2, 1),
         (20, 30, 4, 3, 1, 34, 17, 12, 1, 3, 1)]


def _case(k, w, h, ch, D, dmin, l1, l2, tau1, tau2, it, want_agg):
    rng = np.random.default_rng(40 + k)
    guide = textured_guide(h, w, seed=k, channels=ch)
    cost = (rng.random((D, h, w)) * 300 - 20).astype(np.float32)
    cost.reshape(-1)[rng.permutation(cost.size)[:5]] = np.array([np.nan, np.inf, -np.inf, 255.5, -0.0], np.float32)[:min(5, cost.size)]
    best, disp = smx.init_wta(h, w)
    best[rng.random((h, w)) < 0.2] = np.float32(0.5)             # IN/OUT: some pixels come in with a winner that mostly stays
    disp[best == np.float32(0.5)] = 99
    q = ref.aggregate(guide, cost, l1=l1, l2=l2, tau1=tau1, tau2=tau2, iterations=it)
    wb, wd = best.copy(), disp.copy()
    for z in range(D):                                           # dispSelect: if (best >= q) { dmap = dmin + z; best = q; }
        take = wb >= q[z]
        wb, wd = np.where(take, q[z], wb), np.where(take, np.float32(dmin + z), wd)
    want = {"best.f32": wb, "disp.f32": wd}
    if want_agg:
        want["agg.f32"] = q
    stem = f"case{k}"
    return {"line": f"cross {stem} {w} {h} {ch} {D} {dmin} {l1} {l2} {tau1} {tau2} {it} {want_agg}", "stem": stem, "want": want,
            "inputs": {"guide.u8": guide, "cost.f32": cost, "best_in.f32": best, "disp_in.f32": disp}}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = [_case(k, *c) for k, c in enumerate(CASES)]
    exe = str(tmp_path / "host_cross_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_cross_check.cpp"),
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
        for suffix, want in c["want"].items():
            got = np.fromfile(work / f"{c['stem']}.{suffix}", "<f4").reshape(want.shape)
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), f"{c['line']}: {suffix}: {(~same).sum()} of {same.size} elements differ"
