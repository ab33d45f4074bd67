"""The CPU twins of the mutual-information cost (host/cpu_twins.cpp: mi_histogramOnCPU, mi_costOnCPU) against tests/mi_ref.py,
bit for bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

The twins are what `smx_main --cost mi --host-compare` trusts.  tests/host_mi_check.cpp is the stand-alone program that runs them
(no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files -- the pair, a left map and
its histogram by mi_ref, a table and the two volumes of mi_ref -- and compares the twins' results with them.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_mi
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mi_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

# w, h, size_d, dminl, dminr: one pixel, one row, one column, labels on either side of zero and wholly outside the image
SHAPES = [(1, 1, 1, 0, 0), (1, 1, 3, -1, -1), (40, 1, 7, -3, -3), (1, 9, 2, 0, -1), (5, 4, 12, -6, -5), (33, 6, 9, -8, 0),
          (33, 6, 9, 2, -10), (21, 5, 3, -200, 198), (21, 5, 2, 150, -151), (67, 9, 16, -15, 0)]
MARK = -115.0


def cases():
    out = []
    for k, (w, h, D, dminl, dminr) in enumerate(SHAPES):
        rng = np.random.default_rng(300 + k)
        L, R = (rng.integers(0, 256, size=(h, w), dtype=np.uint8) for _ in range(2))
        if k % 2:                              # few gray levels: the counters reach more than one
            L, R = (L // 64 * 64).astype(np.uint8), (R // 32 * 32).astype(np.uint8)
        disp = rng.integers(-w - 1, w + 2, size=(h, w)).astype(np.float32)
        disp[rng.random((h, w)) < 0.3] = MARK
        hist = ref.histogram(L, R, disp, MARK)
        # the table of that histogram where it has one, else an arbitrary asymmetric one
        table = ref.table(hist) if k % 3 == 0 and hist.any() else rng.integers(0, 256, size=(256, 256), dtype=np.uint8)
        out.append({"stem": f"mi{k}_{w}x{h}x{D}", "line": f"{w} {h} {D} {dminl} {dminr} {MARK}",
                    "files": {"l.u8": L, "r.u8": R, "disp.f32": disp, "hist.u32": hist, "table.u8": table,
                              "wantl.f32": ref.cost(table, L, R, D, dminl), "wantr.f32": ref.cost(table, L, R, D, dminr, right=True)}})
    return out


def _write(work, cs):
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(f"{c['stem']} {c['line']}" for c in cs) + "\n")
    for c in cs:
        for suffix, a in c["files"].items():
            a = np.ascontiguousarray(a)
            a.astype(a.dtype.newbyteorder("<")).tofile(work / f"{c['stem']}.{suffix}")


def _build(tmp_path, build):
    exe = str(tmp_path / "host_mi_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_mi_check.cpp"), os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    return exe


def _run(exe, work):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)


@pytest.mark.parametrize("build", list(BUILDS))
def test_the_twins_equal_the_reference(tmp_path, build):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and `ok` for every case."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = cases()
    exe = _build(tmp_path, build)
    _write(tmp_path / "cases", cs)
    r = _run(exe, tmp_path / "cases")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert [l[3:] for l in r.stdout.splitlines() if l.startswith("ok ")] == [c["stem"] for c in cs]
    assert f"cases {len(cs)}\n" in r.stdout


def test_the_program_sees_a_wrong_volume_and_a_wrong_counter(tmp_path):
    """One cell of one reference volume off by one ulp, one counter of another case off by one: the program names both cases
    and exits 1."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = cases()[4:7]
    bad = cs[1]["files"]["wantr.f32"].copy()
    bad.view(np.uint32)[-1, -1, -1] ^= 1
    cs[1] = dict(cs[1], files=dict(cs[1]["files"], **{"wantr.f32": bad}))
    hist = cs[2]["files"]["hist.u32"].copy()
    hist[255, 255] += 1
    cs[2] = dict(cs[2], files=dict(cs[2]["files"], **{"hist.u32": hist}))
    exe = _build(tmp_path, "plain")
    _write(tmp_path / "cases", cs)
    r = _run(exe, tmp_path / "cases")
    assert r.returncode == 1 and f"ok {cs[0]['stem']}" in r.stdout, r.stdout + r.stderr
    assert f"MISMATCH {cs[1]['stem']} view 1" in r.stdout and f"MISMATCH {cs[2]['stem']} histogram" in r.stdout, r.stdout
