"""The CPU twin of hierarchical belief propagation (host/cpu_twins.cpp: beliefPropagationOnCPU) against tests/bp_ref.py, bit for
bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

tests/host_bp_check.cpp is the stand-alone program that runs it (no libsmx_hip.so, nothing loaded into python): it reads the
cases this module writes as raw files and writes the results beside them; the comparison with the values of bp_ref is made
here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_bp
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bp_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

F32 = np.float32
# w, h, dmin, size_d, step, trunc, iterations, levels, data_scale, the costs' upper end
CASES = [(1, 1, 0, 1, 20, 60, 5, 4, 1.0, 255), (1, 6, -2, 3, 20, 60, 3, 2, 1.0, 62), (6, 1, 3, 2, 7, 7, 1, 4, 1.0, 255),
         (2, 2, -3, 4, 0, 0, 5, 2, 1.0, 62), (5, 3, -4, 5, 1, 4095, 3, 3, 1.0, 255), (7, 9, 0, 4, 4095, 4095, 2, 4, 1.0, 255),
         (9, 7, -4, 5, 3, 0, 3, 2, 1.0, 62), (19, 40, -15, 16, 20, 60, 5, 4, 16.0, 2.5), (33, 6, -69, 70, 20, 60, 0, 4, 1.0, 255),
         (65, 3, -8, 9, 20, 60, 5, 1, 0.5, 300), (129, 70, -15, 16, 20, 60, 5, 8, 1.0, 62)]
SPECIALS = np.array([-1, -0.0, 0.5, 254.999, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40], F32)


def _same(got, want, name):
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ"


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_bp_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_bp_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    lines, checks = [], []
    rng = np.random.default_rng(91)
    for k, (w, h, dmin, D, step, trunc, it, lv, scale, hi) in enumerate(CASES):
        cost = (rng.random((D, h, w)) * hi).astype(F32) if hi < 10 else rng.integers(0, hi + 1, (D, h, w)).astype(F32)
        if k % 4 == 1:          # special values go through the clamp
            cost.reshape(-1)[rng.integers(0, cost.size, max(1, cost.size // 5))] = SPECIALS[rng.integers(0, SPECIALS.size, max(1, cost.size // 5))]
        cost.astype("<f4").tofile(work / f"b{k}.cost.f32")
        want = ref.outputs(cost, step, trunc, it, lv, scale)
        tail = f"{w} {h} {dmin} {D} {step} {trunc} {it} {lv} {scale!r}"
        lines.append(f"bp b{k} {tail}")
        disp = (dmin + want["z"]).astype(F32)
        checks += [(f"b{k}.agg.f32", want["agg"]), (f"b{k}.best.f32", want["best"]), (f"b{k}.disp.f32", disp)]
        if k % 3 == 0:
            shutil.copy(work / f"b{k}.cost.f32", work / f"w{k}.cost.f32")
            lines.append(f"winners w{k} {tail}")
            checks += [(f"w{k}.best.f32", want["best"]), (f"w{k}.disp.f32", disp)]
    (work / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(lines)}\n" in r.stdout
    for name, want in checks:
        got = np.fromfile(work / name, "<f4").reshape(want.shape)
        _same(got, want, name)
