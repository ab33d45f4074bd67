"""The CPU twin of the AD-Census cost (host/cpu_twins.cpp: adcensus_costOnCPU) against tests/adcensus_ref.py, bit for bit,
without a GPU -- once plain and once under -fsanitize=address,undefined.

The twin is what `smx_main --cost adcensus --host-compare` trusts.  tests/host_adcensus_check.cpp is the stand-alone
program that runs it (no libsmx_hip.so, nothing loaded into python): it reads the cases this module writes as raw files --
the images, the tables of smx_adcensus_tables and the volumes of adcensus_ref -- and compares the twin's volumes with them.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_adcensus
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import adcensus_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

# w, h, size_d, dmin, channels, rx, ry, th: one pixel, one row, one column, images smaller than the window, labels on either
# side of zero and wholly outside the image, every channel count, a truncation below and one above the window's bits
SHAPES = [(1, 1, 1, 0, 1, 4, 3, 62), (1, 1, 3, -1, 3, 1, 1, 8), (40, 1, 7, -3, 1, 4, 3, 62), (1, 9, 2, 0, 4, 2, 3, 20),
          (5, 4, 12, -6, 3, 4, 3, 62), (33, 6, 9, -8, 1, 4, 1, 5), (33, 6, 9, 2, 4, 1, 1, 99), (21, 5, 3, -200, 3, 4, 3, 62),
          (21, 5, 2, 150, 1, 2, 1, 9), (67, 9, 16, -15, 4, 4, 3, 40)]
TABLES = [(30.0, 10.0, 127.5), (0.5, 0.5, 2.0 ** 20), (1e6, 1e6, 2.0 ** -20)]


def cases():
    out = []
    for k, (w, h, D, dmin, ch, rx, ry, th) in enumerate(SHAPES):
        rng = np.random.default_rng(100 + k)
        lc, la, scale = TABLES[k % len(TABLES)]
        colour = int(ch != 1)
        gray = [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for _ in range(2)]
        if k % 2:                              # few gray levels: equal neighbours everywhere
            gray = [(g // 64 * 64).astype(np.uint8) for g in gray]
        imgs = gray if ch == 1 else [rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8) for _ in range(2)]
        p = _lib.AdCensusParams()
        p.census.rx, p.census.ry, p.census.th = rx, ry, th
        p.lambda_census, p.lambda_ad, p.scale, p.colour = lc, la, scale, colour
        table = smx.adcensus_tables(p)         # the library's tables, as main.cpp hands them to the twin
        want = ref.cost(imgs[0], imgs[1], gray[0], gray[1], D, dmin, rx=rx, ry=ry, th=th, colour=colour, table=table)
        out.append({"stem": f"adc{k}_{w}x{h}x{D}_c{ch}", "line": f"{w} {h} {D} {dmin} {ch} {rx} {ry} {th} {colour}",
                    "files": {"i1.u8": imgs[0], "i2.u8": imgs[1], "g1.u8": gray[0], "g2.u8": gray[1], "table.f32": table,
                              "want.f32": want}})
    return out


def _write(work, cs):
    work.mkdir()
    (work / "cases.txt").write_text("\n".join(f"{c['stem']} {c['line']}" for c in cs) + "\n")
    for c in cs:
        for suffix, a in c["files"].items():
            a = np.ascontiguousarray(a)
            a.astype(a.dtype.newbyteorder("<")).tofile(work / f"{c['stem']}.{suffix}")


def _build(tmp_path, build):
    exe = str(tmp_path / "host_adcensus_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST,
                           os.path.join(ROOT, "tests", "host_adcensus_check.cpp"), os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    return exe


def _run(exe, work):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)


@pytest.mark.parametrize("build", list(BUILDS))
def test_the_twin_equals_the_reference(tmp_path, build):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and `ok` for every case."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = cases()
    assert {c["line"].split()[4] for c in cs} == {"1", "3", "4"}
    exe = _build(tmp_path, build)
    _write(tmp_path / "cases", cs)
    r = _run(exe, tmp_path / "cases")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert [l[3:] for l in r.stdout.splitlines() if l.startswith("ok ")] == [c["stem"] for c in cs]
    assert f"cases {len(cs)}\n" in r.stdout


def test_the_program_sees_a_wrong_volume(tmp_path):
    """One cell of one reference volume off by one ulp: the program names the case and exits 1."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    cs = cases()[4:6]
    bad = cs[1]["files"]["want.f32"].copy()
    bad.view(np.uint32)[-1, -1, -1] ^= 1
    cs[1] = dict(cs[1], files=dict(cs[1]["files"], **{"want.f32": bad}))
    exe = _build(tmp_path, "plain")
    _write(tmp_path / "cases", cs)
    r = _run(exe, tmp_path / "cases")
    assert r.returncode == 1 and f"ok {cs[0]['stem']}" in r.stdout and f"MISMATCH {cs[1]['stem']}" in r.stdout, r.stdout + r.stderr
