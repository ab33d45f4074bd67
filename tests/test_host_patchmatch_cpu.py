"""The CPU twins of PatchMatch stereo (host/cpu_twins.cpp: patchMatchOnCPU, pmPlaneCostOnCPU) against tests/patchmatch_ref.py,
bit for bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --aggregation patchmatch --host-compare` trusts.  tests/host_patchmatch_check.cpp is the stand-alone
program that runs it (no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files and
writes the twins' outputs beside them; the comparison with the values of patchmatch_ref is made here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_patchmatch
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import patchmatch_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT
from test_patchmatch_cpu import random_pair

F32 = np.float32
# w, h, D, dminl, dminr, radius, gamma, iterations, max_slope, seed: one pixel, one row, one column, every +-5 neighbour outside,
# odd sizes, one label, many labels, positive dmin, the fronto-parallel search, the largest radius, a window taller than the image
CASES = [(1, 1, 6, -5, 0, 2, 10.0, 2, 2.0, 0),
         (23, 1, 4, -3, 0, 1, 10.0, 2, 2.0, 1),
         (1, 17, 4, -3, 0, 1, 10.0, 2, 2.0, 2),
         (6, 6, 6, -5, 0, 2, 10.0, 2, 2.0, 3),
         (37, 19, 6, -5, 0, 2, 4.5, 2, 2.0, 4),
         (21, 9, 1, -2, 0, 2, 10.0, 2, 2.0, 5),
         (15, 7, 300, -299, 0, 1, 10.0, 1, 8.0, 6),
         (21, 9, 6, 3, 2, 2, 10.0, 2, 0.5, 7),
         (21, 9, 6, -5, 0, 2, 10.0, 3, 0.0, 4294967295),
         (20, 12, 5, -4, 0, 17, 25.0, 1, 2.0, 9),
         (30, 5, 5, -4, 0, 8, 10.0, 1, 2.0, 10)]
# the default parameters of the library (smx_default_params), which the stand-alone program's smx_config restates
CC = ref.cost_const(0.9, 7, 2)


def _case(k, w, h, D, dminl, dminr, radius, gamma, iterations, slope, seed):
    rng = np.random.default_rng(900 + k)
    left, right = random_pair(rng, h, w, -2 if dminl < 0 else 3)
    pm = ref.PMParams(radius, gamma, iterations, slope, seed)
    want = ref.patchmatch(left, right, D, dminl, dminr, pm, CC)
    tail = f"{w} {h} {D} {dminl} {dminr} {radius} {gamma!r} {iterations} {slope!r} {seed}"
    cases = [{"line": f"search s{k} {tail}", "stem": f"s{k}", "inputs": {"left.u8": left, "right.u8": right},
              "want": {k2: want[k2] for k2 in ("planes", "cost", "disp", "label")}}]
    # the plane cost alone, on random planes, some outside the labels, a NaN and an infinity among them
    planes = np.empty((2, 3, h, w), F32)
    planes[:, :2] = rng.uniform(-2.5, 2.5, (2, 2, h, w))
    planes[0, 2] = rng.uniform(dminl - 1.5, dminl + D + 0.5, (h, w))
    planes[1, 2] = rng.uniform(dminr - 1.5, dminr + D + 0.5, (h, w))
    planes[0, 2, 0, 0], planes[1, 0, h - 1, w - 1] = np.nan, np.inf
    cost = np.stack([ref.plane_cost_map(left, right, dminl, D, pm, CC, planes[0]),
                     ref.plane_cost_map(right, left, dminr, D, pm, CC, planes[1])])
    cases.append({"line": f"cost c{k} {tail}", "stem": f"c{k}", "inputs": {"left.u8": left, "right.u8": right, "planes.f32": planes},
                  "want": {"cost": cost}})
    return cases


@pytest.fixture(scope="module")
def cases():
    return [c for k, args in enumerate(CASES) for c in _case(k, *args)]


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twins_equal_the_reference(build, cases, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_patchmatch_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_patchmatch_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(c["line"] for c in cases) + "\n")
    for c in cases:
        for suffix, a in c["inputs"].items():
            a = np.ascontiguousarray(a)
            a.astype(a.dtype.newbyteorder("<")).tofile(work / f"{c['stem']}.{suffix}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(cases)}\n" in r.stdout
    for c in cases:
        for name, want in c["want"].items():
            got = np.fromfile(work / f"{c['stem']}.{name}.f32", "<f4").reshape(want.shape)
            same = got.view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
            assert same.all(), f"{c['line']} {name}: {(~same).sum()} of {same.size} elements differ"
