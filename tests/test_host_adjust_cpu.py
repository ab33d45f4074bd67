"""The CPU twin of the depth-discontinuity adjustment (host/cpu_twins.cpp: discontinuityAdjustOnCPU) against
tests/adjust_ref.py, bit for bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --adjust --host-compare` trusts.  tests/host_adjust_check.cpp is the stand-alone program that runs it
(no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files and writes the twin's output
beside them; the comparison with the values of adjust_ref is made here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_adjust
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adjust_ref as ref
from test_adjust_cpu import random_case
from test_host_twins_cpu import BUILDS, HOST, ROOT

F32 = np.float32
# w, h, D, dmin, tau_e, vertical, iterations, subpix_mode: one pixel, one row, one column, one label, the label range's ends, every
# number of rounds at the ends of its range, both axes, both fits and none, dmin negative, zero and positive
CASES = [(1, 1, 1, 0, 1, 1, 1, 0),
         (40, 1, 3, -2, 1, 1, 2, 1),
         (1, 23, 4, 0, 2, 1, 8, 2),
         (33, 21, 1, -3, 1, 1, 3, 1),
         (64, 24, 8, -4, 2, 1, 1, 2),
         (31, 17, 5, 0, 5, 0, 3, 1),
         (20, 30, 16, 1, 1, 0, 8, 0),
         (45, 19, 6, -8, 3, 1, 4, 2),
         (9, 7, 512, -300, 100, 1, 2, 1)]


def _case(k, w, h, D, dmin, tau_e, vertical, iterations, mode):
    rng = np.random.default_rng(60 + k)
    d, vol = random_case(rng, h, w, dmin, D, block=(2, 3))
    sub = rng.normal(size=(h, w)).astype(F32) if mode else None
    want = ref.adjust(d, vol, dmin, tau_e, vertical, iterations, mode=mode or None, sub=sub)
    want, wsub = want if mode else (want, None)
    stem = f"case{k}"
    inputs = {"disp.f32": d, "agg.f32": vol}
    if mode:
        inputs["sub.f32"] = sub
    return {"line": f"adjust {stem} {w} {h} {D} {dmin} {tau_e} {vertical} {iterations} {mode}", "stem": stem, "want": want,
            "wsub": wsub, "inputs": inputs, "changed": int((want.view(np.uint32) != d.view(np.uint32)).sum())}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = [_case(k, *c) for k, c in enumerate(CASES)]
    assert sum(c["changed"] > 0 for c in cs) >= 6           # the cases do something
    exe = str(tmp_path / "host_adjust_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_adjust_check.cpp"),
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
        for name, want in (("adjusted", c["want"]), ("subout", c["wsub"])):
            if want is None:
                continue
            got = np.fromfile(work / f"{c['stem']}.{name}.f32", "<f4").reshape(want.shape)
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), f"{c['line']} {name}: {(~same).sum()} of {same.size} elements differ"
