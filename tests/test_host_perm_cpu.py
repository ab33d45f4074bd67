"""The CPU twin of the permeability filter (host/cpu_twins.cpp: permeabilityOnCPU) and the host arithmetic behind smx_perm_table
(csrc/smx_perm_host.h: the code the library's entries run) against tests/perm_ref.py, bit for bit, without a GPU -- once plain and
once under -fsanitize=address,undefined.

tests/host_perm_check.cpp is the stand-alone program that runs them (no libsmx_hip.so, nothing loaded into python): it reads the
cases this module writes as raw files and writes the results beside them; the comparison with the values of perm_ref is made
here.  The shapes are 1 x 1, 2 x 1, 1 x 2, 7 x 5, 19 x 40 and 129 x 70.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_perm
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import perm_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

F32 = np.float32
SIGMAS = [32.0, 16.0, 64.0, 0.001, 0.011, 0.012, 7.3, 1e6]
# w, h, channels, dmin, size_d, sigma
FILTER = [(1, 1, 1, 0, 1, 32.0), (2, 1, 3, -1, 2, 32.0), (1, 2, 4, 3, 3, 8.0), (7, 5, 1, -3, 3, 0.012), (7, 5, 3, -3, 3, 0.011), (7, 5, 1, 2, 1, 32.0),
          (19, 40, 4, -15, 16, 32.0), (19, 40, 1, -16, 17, 0.001), (129, 70, 1, -15, 16, 32.0), (129, 70, 3, 0, 5, 64.0)]


def _volume(rng, w, h, size_d, k):
    v = (rng.integers(-3, 4, (size_d, h, w)) * 0.5).astype(F32) if k % 2 else rng.standard_normal((size_d, h, w)).astype(F32)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = -0.0
    # (a NaN or an infinity takes its whole slice with it -- along its row, then down every column: one slice each)
    for z, val in zip(rng.permutation(size_d), (np.nan, np.inf, -np.inf) if size_d >= 4 else ()):
        v[z, rng.integers(0, h), rng.integers(0, w)] = val
    return v


def _guide(rng, w, h, ch):
    base = rng.integers(0, 256, (h // 7 + 1, w // 5 + 1, ch)).astype(np.int64)
    g = np.kron(base, np.ones((7, 5, 1), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w, ch))
    return np.clip(g, 0, 255).astype(np.uint8)


def _same(got, want, name):
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ"


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twin_equals_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_perm_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_perm_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    lines, checks = [], []
    rng = np.random.default_rng(78)
    for k, sigma in enumerate(SIGMAS):
        lines.append(f"table t{k} {sigma!r}")
        checks.append((f"t{k}.t.f32", ref.table(sigma)))
    for k, (w, h, ch, dmin, size_d, sigma) in enumerate(FILTER):
        vol, guide = _volume(rng, w, h, size_d, k), _guide(rng, w, h, ch)
        if size_d == 1 and w > 1:
            vol[0, h // 2, w // 2] = np.nan             # the NaN reaches every pixel of its slice: no pixel has a winner
        vol.astype("<f4").tofile(work / f"f{k}.vol.f32")
        guide.tofile(work / f"f{k}.guide.u8")
        out = ref.filter_volume(vol, guide, sigma)
        z, c0 = ref.winners(out)
        best = np.where(z >= 0, c0, F32(np.nan)).astype(F32)
        lines.append(f"filter f{k} {w} {h} {ch} {dmin} {size_d} {sigma!r}")
        checks += [(f"f{k}.out.f32", out), (f"f{k}.best.f32", best), (f"f{k}.disp.f32", ref.label_map(z, dmin))]
        if k % 3 == 0:
            for ext in ("vol.f32", "guide.u8"):
                shutil.copy(work / f"f{k}.{ext}", work / f"w{k}.{ext}")
            lines.append(f"winners w{k} {w} {h} {ch} {dmin} {size_d} {sigma!r}")
            checks += [(f"w{k}.best.f32", best), (f"w{k}.disp.f32", ref.label_map(z, dmin))]
    (work / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(lines)}\n" in r.stdout
    for name, want in checks:
        got = np.fromfile(work / name, "<f4").reshape(want.shape)
        _same(got, want, name)


def test_the_library_entries_equal_the_reference():
    """smx_default_perm_params, smx_perm_table and smx_perm_workspace_bytes of the built library (not sanitised: it is loaded into
    python) -- no device call"""
    from stereo_matching_cuda_amd import _lib
    assert _lib.default_perm_params().sigma == ref.DEFAULT_SIGMA
    for sigma in SIGMAS:
        p = _lib.default_perm_params()
        p.sigma = sigma
        _same(np.array(_lib.perm_table(p), F32), ref.table(sigma), f"table {sigma}")
    assert _lib.lib().smx_perm_workspace_bytes(129, 70, 16, 2) == 2 * 129 * 70 * 4 * (2 + 2 * 16)
    assert _lib.lib().smx_perm_workspace_bytes(129, 70, 16, 3) == 0
