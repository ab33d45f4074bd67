"""The CPU twins of cross-scale aggregation (host/cpu_twins.cpp: pyrDownOnCPU, crossScaleOnCPU) and the host arithmetic behind
smx_cscale_weights / smx_cscale_level (csrc/smx_cscale_host.h: the code the library's entries run) against tests/cscale_ref.py,
bit for bit, without a GPU -- once plain and once under -fsanitize=address,undefined.

tests/host_cscale_check.cpp is the stand-alone program that runs them (no libsmx_hip.so, nothing loaded into python): it reads the
cases this module writes as raw files and writes the results beside them; the comparison with the values of cscale_ref is made
here.  The shapes are 5 x 3, 19 x 40 and 129 x 70.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k host_cscale
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cscale_ref as ref
from test_host_twins_cpu import BUILDS, HOST, ROOT

F32 = np.float32
SHAPES = [(5, 3), (19, 40), (129, 70)]
# w, h, dmin, size_d, scales, lambda
COMBINE = [(5, 3, -1, 2, 3, 0.3), (5, 3, 3, 1, 1, 1.0), (19, 40, -15, 16, 5, 1.0), (19, 40, -16, 17, 2, 0.0), (129, 70, -15, 16, 4, 1.0),
           (129, 70, 0, 17, 3, 0.3)]
WEIGHTS = [(s, lam) for s in range(1, 6) for lam in (0.0, 0.3, 1.0, 2.5, 1e-3, 1e6)]


def _levels(rng, w, h, dmin, size_d, scales):
    out = []
    for s in range(scales):
        ws, hs, _, ds = ref.level(w, h, dmin, size_d, s)
        v = (rng.integers(-3, 4, (ds, hs, ws)) * 0.5).astype(F32) if s == 0 else rng.standard_normal((ds, hs, ws)).astype(F32)
        flat = v.reshape(-1)
        for val in (np.nan, np.inf, -0.0):
            flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = val
        out.append(v)
    out[0][:, 0, 0] = np.nan            # a pixel without a winner
    return out


def _same(got, want, name):
    if want.dtype == F32:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements differ"


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_twins_equal_the_reference(build, tmp_path):
    """Exit status 0, a clean stderr (no sanitizer report in the sanitized build, which is the program itself, nothing
    preloaded), and every output equal to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_cscale_check")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "host_cscale_check.cpp"),
                           os.path.join(HOST, "cpu_twins.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    lines, checks = [], []
    rng = np.random.default_rng(77)
    for k, ((w, h), ch) in enumerate((s, c) for s in SHAPES + [(1, 1), (2, 1), (1, 2)] for c in (1, 3, 4)):
        img = rng.integers(0, 256, (h, w, ch)).astype(np.uint8)
        img.tofile(work / f"pyr{k}.src.u8")
        lines.append(f"pyr pyr{k} {w} {h} {ch}")
        checks.append((f"pyr{k}.dst.u8", ref.pyr_down(img)))
    for k, (s, lam) in enumerate(WEIGHTS):
        lines.append(f"weights wt{k} {s} {lam!r}")
        checks.append((f"wt{k}.wt.f32", ref.weights(s, lam)))
    for k, (w, h, dmin, size_d, scales, lam) in enumerate(COMBINE):
        lv = _levels(rng, w, h, dmin, size_d, scales)
        for s, v in enumerate(lv):
            v.astype("<f4").tofile(work / f"cs{k}.level{s}.f32")
        lines.append(f"combine cs{k} {w} {h} {dmin} {size_d} {scales} {lam!r}")
        out = ref.combine(lv, dmin, size_d, lam)
        z, c0 = ref.winners(out)
        assert z[0, 0] == -1 and (z >= 0).sum() >= z.size // 2
        checks += [(f"cs{k}.out.f32", out), (f"cs{k}.best.f32", np.where(z >= 0, c0, F32(np.nan)).astype(F32)),
                   (f"cs{k}.disp.f32", (dmin + np.maximum(z, 0)).astype(F32))]
    (work / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and r.stderr == "", r.stderr[-4000:]
    assert f"cases {len(lines)}\n" in r.stdout
    for name, want in checks:
        got = np.fromfile(work / name, "<f4" if want.dtype == F32 else np.uint8).reshape(want.shape)
        _same(got, want, name)


def test_the_library_entries_equal_the_reference():
    """smx_cscale_weights and smx_cscale_level of the built library (not sanitised: it is loaded into python) -- no device call"""
    from stereo_matching_cuda_amd import _lib
    for s, lam in WEIGHTS:
        p = _lib.default_cscale_params()
        p.scales, p.lambda_ = s, lam
        _same(np.array(_lib.cscale_weights(p), F32), ref.weights(s, lam), f"weights {s} {lam}")
    for (w, h), dmin, size_d, s in ((sh, d, n, s) for sh in SHAPES for d in (-15, -16, -1, 0, 3) for n in (1, 2, 16, 17)
                                    for s in range(5)):
        assert _lib.cscale_level(w, h, dmin, size_d, s) == ref.level(w, h, dmin, size_d, s)
