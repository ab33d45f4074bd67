"""What the tests of the drop-in main (`smx_main`, host/main.cpp) share: the one build of the binary, running it on a pair written
as PNGs, decoding and checking the files it writes, the two shapes of test every option has (its default value is a no-op; a
bad use is refused), and the numpy / oracle restatement of the stages behind the winner-take-all.  A plain module: the
fixtures `binary` and `main_cases` are imported from here by the modules that use them.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import ref_fixtures as rf
import speckle_ref
import subpix_ref
import uniq_ref
import wmf_ref

ROOT = rf.ROOT
BIN = os.path.join(ROOT, "stereo_matching_cuda_amd", "_build", "smx_main")

# file name -> the expected map it is the image of (u8 maps are written as they are, f32 maps through the normaliser)
PNGS = {"image_left": "grayl", "image_right": "grayr", "image_mean_left": "meanl", "image_mean_right": "meanr",
        "best_costl": "bestl", "best_costr": "bestr", "cost_lminus15": "cost0l", "cost_rminus15": "cost0r",
        "occlu_mapl": "occlusion", "disparity_mapl": "dmapl", "disparity_mapr": "dmapr", "occlu_mapl_filled": "filled"}
# the maps of the opt-in stages: written exactly when the stage runs
OPTIONAL_PNGS = {"occlu_mapl_unique": "unique", "occlu_mapl_despeckled": "despeckled", "occlu_mapl_wmf": "refined"}


# ---- the binary ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build_main():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "stereo_matching_cuda_amd", "host")])
    assert os.path.exists(BIN)
    return BIN


@pytest.fixture(scope="module")
def binary():
    return build_main()


@pytest.fixture(scope="module")
def main_cases():
    """This module, with the binary built."""
    build_main()
    return sys.modules[__name__]


def write_png(path, a):
    """(h, w) u8 -> gray, (h, w, 3) -> RGB, (h, w, 4) -> RGBA"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.ndim == 2 or a.shape[2] in (3, 4), a.shape
    Image.fromarray(a).save(path)
    return str(path)


def read_pfm(path):
    """(header lines, rows top-down).  The file holds the rows bottom-up."""
    raw = open(path, "rb").read()
    parts = raw.split(b"\n", 3)
    w, h = (int(t) for t in parts[1].split())
    assert len(parts[3]) == 4 * w * h, (len(parts[3]), w, h)
    return parts[:3], np.ascontiguousarray(np.frombuffer(parts[3], "<f4").reshape(h, w)[::-1])


def run_main(binary, tmp_path, left, right, positional, flags=(), cwd=None, outdir=None, timeout=300):
    """Writes the pair as PNGs, runs `smx_main L R <positional> [flags] --pfm F --png16 G`, returns the finished process and
    the decoded files: {"png": {name: array}, "pfm": (header, map), "png16": array} (whatever exists)."""
    ldir = tmp_path / "in"
    ldir.mkdir(exist_ok=True)
    L, R = write_png(ldir / "left.png", left), write_png(ldir / "right.png", right)
    out = outdir if outdir is not None else tmp_path / "out"
    out.mkdir(exist_ok=True)
    pfm, p16 = tmp_path / "disp.pfm", tmp_path / "disp16.png"
    cmd = [binary, L, R] + [str(a) for a in positional] + ([str(out)] if outdir is None else []) + list(flags) + \
          ["--pfm", str(pfm), "--png16", str(p16)]
    r = subprocess.run(cmd, cwd=cwd or tmp_path, capture_output=True, text=True, timeout=timeout)
    files = {"png": {f[:-4]: np.asarray(Image.open(out / f)) for f in sorted(os.listdir(out)) if f.endswith(".png")}}
    if pfm.exists():
        files["pfm"] = read_pfm(pfm)
    if p16.exists():
        a = np.asarray(Image.open(p16))
        assert a.min() >= 0 and a.max() <= 65535
        files["png16"] = a.astype(np.uint16)
    return r, files


def run_ok(tmp_path, left, right, positional, flags=(), timeout=120):
    """run_main of a command line that must succeed: exit status 0 and no mismatch reported by a self-check."""
    r, files = run_main(build_main(), tmp_path, left, right, positional, flags, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "error at element" not in r.stdout, r.stdout[-2000:]
    return r, files


# ---- checking what it wrote ------------------------------------------------------------------------------------------------
def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), f"{what}: {rf.first_difference(got, want)}"


def check_twelve(orc, files, e, what):
    assert set(PNGS) <= set(files["png"]), (what, sorted(files["png"]))
    for fname, key in PNGS.items():
        want = e[key] if e[key].dtype == np.uint8 else orc.write_mat_u8(e[key])
        same_bits(files["png"][fname], want, f"{what} {fname}.png")


def check_disparity_files(files, final, w, h, what):
    """--pfm: header Pf / w h / a negative scale, rows bottom-up, -final bit for bit; --png16: clip(-final * 256, 0, 65535),
    truncated."""
    head, d = files["pfm"]
    assert head[0] == b"Pf" and head[1] == b"%d %d" % (w, h) and float(head[2]) < 0, (what, head)
    same_bits(d, -np.asarray(final, np.float32), what + " pfm")
    want16 = np.clip(-np.asarray(final, np.float32) * np.float32(256.0), np.float32(0.0), np.float32(65535.0)).astype(np.uint16)
    same_bits(files["png16"], want16, what + " png16")


def check_outputs(orc, files, e, w, h, what, mean_empty=False):
    """The twelve images, the maps of the opt-in stages (present exactly when `e` holds their key) and the pfm / png16 files
    of e["final"]."""
    check_twelve(orc, files, e, what)
    if mean_empty:
        assert not files["png"]["image_mean_left"].any() and not files["png"]["image_mean_right"].any(), what
    for fname, key in OPTIONAL_PNGS.items():
        if key in e:
            same_bits(files["png"][fname], orc.write_mat_u8(e[key]), f"{what} {fname}.png")
        else:
            assert fname not in files["png"], (what, fname)
    check_disparity_files(files, e["final"], w, h, what)


def check_ok_lines(r, lines):
    for line, count in lines.items():
        assert r.stdout.count(line) == count, (line, count, r.stdout[-2000:])


def assert_same_files_as_plain(tmp_path, left, right, positional, flags):
    """An option at its default value: the twelve images, the pfm and the png16 byte for byte those of a run without it.
    -> the directory of the plain run."""
    blobs = []
    for sub, fl in (("plain", []), ("option", flags)):
        d = tmp_path / sub
        d.mkdir()
        run_ok(d, left, right, positional, fl)
        names = sorted(os.listdir(d / "out"))
        assert names == sorted(f + ".png" for f in PNGS), names
        blobs.append({n: (d / "out" / n).read_bytes() for n in names})
        blobs[-1].update({n: (d / n).read_bytes() for n in ("disp.pfm", "disp16.png")})
    assert blobs[0].keys() == blobs[1].keys()
    for n in blobs[0]:
        assert blobs[0][n] == blobs[1][n], n
    return tmp_path / "plain"


def assert_refused(tmp_path, left, right, positional, flags, names, timeout=60):
    """A command line that must be refused: exit status 2, stderr names the option (one of `names`), nothing written."""
    r, files = run_main(build_main(), tmp_path, left, right, positional, flags, timeout=timeout)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert any(n in r.stderr for n in ([names] if isinstance(names, str) else names)), r.stderr
    assert not files["png"] and "pfm" not in files and "png16" not in files
    return r


# ---- what the main computes behind the winner-take-all, in numpy and the oracle alone ------------------------------------------
def finish_chain(orc, e, d_lo, D, z=None, best=None, sec=None, nbr=None, uniqueness=None, speckle=None, subpixel=None,
                 wmf=None):
    """`e` holds the maps up to dmapl / dmapr (and grayl); z, best, sec, nbr are the left view's winners, their costs, the
    second-best costs and the neighbours (lo, hi).  Adds occlusion, unique / despeckled / sub_filled / refined where the
    options ask for them, filled and final: LR check -> uniqueness PCT -> speckle (size, diff) -> fill -> sub-pixel fit /
    weighted median mode."""
    e["occlusion"] = orc.detect_occlusion(e["dmapl"], e["dmapr"], d_lo - 100)
    kept = e["occlusion"]
    if uniqueness:
        ratio = np.float32(uniqueness) / (np.float32(100.0) - np.float32(uniqueness))       # main.cpp: pct / (100.0f - pct)
        kept = e["unique"] = uniq_ref.apply(kept, z >= 0, best, sec, ratio, d_lo, d_lo - 100)[0]
    if speckle:
        kept = e["despeckled"] = speckle_ref.speckle_filter(kept, d_lo, d_lo - 100, *speckle)
    e["filled"] = e["final"] = orc.fill_occlusion(kept, d_lo)
    if subpixel:
        _, e["sub_filled"] = subpix_ref.maps(subpix_ref.MODES[subpixel], z, best, nbr[0], nbr[1], e["dmapl"], kept, e["filled"],
                                             d_lo)
        e["final"] = e["sub_filled"]
    if wmf:
        e["refined"] = wmf_ref.weighted_median(e["grayl"], e["filled"], d_lo, D, kept if wmf == "occluded" else None)
        e["final"] = e["refined"]
    return e
