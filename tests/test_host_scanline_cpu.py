"""The CPU twin of the scan-line optimiser (host/cpu_twins.cpp: scanline_optimizeOnCPU) against tests/scanline_ref.py, bit for
bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --aggregation scanline / cross-scanline --host-compare` trusts.  tests/host_scanline_check.cpp is the
stand-alone program that runs it (no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw
files and writes the twin's outputs beside them; the comparison with the values of scanline_ref is made here.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_scanline
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scanline_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

# w, h, channels, D, dmin, p1, p2, tau_so, paths, want_agg, cost kind: one pixel, one row, one column, every channel count,
# w < h with eight paths, every partner outside on either side, a range that straddles a border, the ends of the penalty and
# threshold ranges, special cost values
CASES = [(1, 1, 1, 1, 0, 127, 382, 15, 4, 1, "plain"),
         (40, 1, 3, 3, -2, 127, 382, 15, 8, 1, "plain"),
         (1, 23, 4, 2, 0, 3, 3, 1, 8, 0, "plain"),
         (9, 21, 3, 7, -3, 40, 400, 15, 8, 1, "plain"),
         (33, 12, 1, 9, -8, 0, 0, 15, 4, 1, "special"),
         (20, 10, 4, 5, 20, 7, 4095, 12, 8, 1, "plain"),
         (20, 10, 3, 5, -25, 4095, 4095, 20, 4, 1, "plain"),
         (31, 9, 3, 12, 25, 10, 120, 256, 8, 0, "special"),
         (24, 8, 3, 8, -4, 39, 39, 13, 8, 1, "low")]


def _case(k, w, h, ch, D, dmin, p1, p2, tau, paths, want_agg, kind):
    rng = np.random.default_rng(90 + k)
    own, other = ((100 + rng.integers(0, 26, (h, w, ch))).astype(np.uint8) for _ in range(2))
    if ch == 4:
        own[:, :, 3], other[:, :, 3] = rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w))
    cost = rng.integers(0, 64 if kind == "low" else 256, (D, h, w)).astype(np.float32)
    if kind == "special":
        specials = np.array([-1, -0.0, 0.5, 254.999, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, 1e-40], np.float32)
        mask = rng.random((D, h, w)) < 0.3
        cost[mask] = specials[rng.integers(0, specials.size, int(mask.sum()))]
    want = ref.outputs(own, other, cost, dmin, p1=p1, p2=p2, tau_so=tau, paths=paths)
    stem = f"case{k}"
    return {"line": f"scanline {stem} {w} {h} {ch} {D} {dmin} {p1} {p2} {tau} {paths} {want_agg}", "stem": stem,
            "inputs": {"own.u8": own, "other.u8": other, "cost.f32": cost}, "want_agg": want_agg,
            "want": {"best": want["best"], "disp": (dmin + want["z"]).astype(np.float32), "agg": want["agg"]},
            "edges": int(ref.edge_count(own, other, 1, 0, dmin, D, tau).max())}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = [_case(k, *c) for k, c in enumerate(CASES)]
    assert sum(c["edges"] == 2 for c in cs) >= 3 and sum(c["edges"] == 0 for c in cs) >= 1     # the cases lower penalties
    exe = str(tmp_path / "host_scanline_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_scanline_check.cpp"),
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
        for name in ("best", "disp") + (("agg",) if c["want_agg"] else ()):
            want = c["want"][name]
            got = np.fromfile(work / f"{c['stem']}.{name}.f32", "<f4").reshape(want.shape)
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), f"{c['line']} {name}: {(~same).sum()} of {same.size} elements differ"
        if not c["want_agg"]:
            assert not (work / f"{c['stem']}.agg.f32").exists()
