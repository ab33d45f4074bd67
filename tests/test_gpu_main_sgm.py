"""The drop-in main with semi-global matching (`smx_main L R DMIN DMAX OUTDIR --aggregation sgm [--sgm-p P1,P2]
[--sgm-paths 4|8] ...`): every file it writes against a chain of references alone -- tests/census_ref.py or the oracle's
cost volume, tests/sgm_ref.py, the oracle's LR check, tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py /
tests/wmf_ref.py; the 8-bit images are oracle.write_mat_u8 of the expected map.  Nothing expected comes from the library
or the binary.  With --host-compare the run also executes sgm_aggregateOnCPU (host/cpu_twins.cpp, held to sgm_ref on the
CPU by tests/test_host_twins_cpu.py) and the check_errors wiring of host/main.cpp around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_sgm
"""
import os
import subprocess

import numpy as np
import pytest

from stereo_matching_cuda_amd import synth

import census_ref
import sgm_ref
from main_harness import (Image, assert_refused, assert_same_files_as_plain, build_main, check_ok_lines, check_outputs,
                          finish_chain, main_cases, run_ok, write_png)  # noqa: F401  (main_cases: a fixture)

pytestmark = pytest.mark.gpu

SPK = (30, 1.0)
#        name: (w, h, the size_d the pair is generated with, seed, d_lo, d_hi)
SCENES = {"main": (129, 70, 70, 4711, -69, 0),        # the shape of the scene of tests/test_gpu_sgm.py
          "x0": (61, 23, 6, 11, -5, 6),               # d_hi != 0: the right volume starts at -d_hi, not at 0
          "d256": (40, 6, 16, 5, -255, 0)}            # 256 labels: the largest the gate admits (4 values per lane)


def rgb_pair(orc, name):
    """(left RGB, right RGB, the gray images expected of them): the idiom of _rgb_pair of tests/test_gpu_census.py."""
    w, h, D, seed = SCENES[name][:4]
    gl, gr = synth.gen_pair(w, h, D, seed)
    rng = np.random.default_rng(seed + 1)
    left, right = (np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8) for g in (gl, gr))
    left[..., 1] += rng.integers(0, 3, size=(h, w), dtype=np.uint8)
    return left, right, orc.gray(left), orc.gray(right)


def chain(orc, gl, gr, d_lo, d_hi, cost="census", cp=census_ref.DEFAULTS, sp=(10, 120, 8), speckle=None, subpixel=None,
          wmf=None):
    """What smx_main --aggregation sgm computes, from the references alone: {key: array}, the keys of PNGS of
    tests/main_harness.py plus despeckled / sub_filled / refined / final where the options ask for them."""
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    if cost == "census":
        vols = [census_ref.census_cost(a, b, D, dm, *cp) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    else:
        vols = [orc.cost_volume(a, b, D, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    sl, sr = (sgm_ref.outputs(v, *sp) for v in vols)
    e = {"grayl": gl, "grayr": gr, "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr),      # SGM has no mean images
         "cost0l": vols[0][0].copy(), "cost0r": vols[1][0].copy(), "bestl": sl["best"], "bestr": sr["best"],
         "dmapl": (dmin[0] + sl["z"]).astype(np.float32), "dmapr": (dmin[1] + sr["z"]).astype(np.float32)}
    return finish_chain(orc, e, d_lo, D, z=sl["z"], best=sl["best"], nbr=sl["nbr"], speckle=speckle, subpixel=subpixel, wmf=wmf)


def build_scenes(orc):
    """name -> (left RGB, right RGB, gray l, gray r, d_lo, d_hi, {configuration: chain(...)}), with the conditions that
    keep the tests from checking nothing asserted on the references alone."""
    out = {}
    for name, (w, h, _, _, d_lo, d_hi) in SCENES.items():
        left, right, gl, gr = rgb_pair(orc, name)
        assert gl.shape == (h, w) and d_hi - d_lo + 1 <= 256
        e = {"default": chain(orc, gl, gr, d_lo, d_hi)}
        out[name] = (left, right, gl, gr, d_lo, d_hi, e)
        d = e["default"]
        dropped = int((d["occlusion"] == d_lo - 100).sum())
        assert 0 < dropped < w * h, (name, dropped)                 # the LR check invalidates some pixels, not all
        assert np.any(d["filled"] != d["occlusion"])
        for k in ("dmapl", "dmapr"):
            assert len(np.unique(d[k])) >= 2, (name, k)
        if -d_lo < w:                                               # (else slice 0 has no partner inside the image)
            assert np.any(d["cost0l"] != d["cost0l"].flat[0]) and np.any(d["cost0r"] != d["cost0r"].flat[0]), name
    left, right, gl, gr, d_lo, d_hi, e = out["main"]
    assert (d_lo, d_hi) == (-69, 0) and out["x0"][5] != 0 and out["d256"][5] - out["d256"][4] + 1 == 256
    e["reference"] = chain(orc, gl, gr, d_lo, d_hi, cost="reference", sp=(5, 40, 4))
    e["spk_sub"] = chain(orc, gl, gr, d_lo, d_hi, cp=(2, 1, 9), speckle=SPK, subpixel="parabola")
    e["spk_wmf"] = chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, wmf="occluded")
    e["wmf_all"] = chain(orc, gl, gr, d_lo, d_hi, wmf="all")
    for k in ("dmapl", "dmapr", "bestl", "cost0l"):                 # the reference cost gives another result
        assert np.any(e["reference"][k] != e["default"][k]), k
    for k in ("spk_sub", "spk_wmf"):
        assert np.any(e[k]["despeckled"] != e[k]["occlusion"]), k   # the speckle filter changed something
        assert np.any(e[k]["filled"] != orc.fill_occlusion(e[k]["occlusion"], d_lo)), k
    assert np.any(e["spk_sub"]["sub_filled"] != np.trunc(e["spk_sub"]["sub_filled"]))       # non-integer disparities
    assert np.any(e["spk_sub"]["dmapl"] != e["default"]["dmapl"])                          # another census window
    for k in ("spk_wmf", "wmf_all"):
        assert np.any(e[k]["refined"] != e[k]["filled"]), k
    assert np.any(e["spk_wmf"]["refined"] != chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, wmf="all")["refined"])
    return out


@pytest.fixture(scope="module")
def scenes(orc):
    return build_scenes(orc)


def run(tmp_path, scene, flags, timeout=120):
    left, right, _, _, d_lo, d_hi, _ = scene
    return run_ok(tmp_path, left, right, [d_lo, d_hi], flags, timeout=timeout)


def check_all(orc, files, e, gl, what):
    check_outputs(orc, files, e, gl.shape[1], gl.shape[0], what, mean_empty=True)


SELF_CHECKS = {"Grayscale ok!": 2, "Semi-global matching ok!": 1, "Occlusion ok!": 1}


# ---- runs that must succeed ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_sgm_defaults(orc, main_cases, scenes, tmp_path, host_compare):
    """Census 9x7 th 62, p 10,120, 8 paths: the twelve images, empty mean images, the census cost slices."""
    scene = scenes["main"]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm"] + (["--host-compare"] if host_compare else []))
    check_all(orc, files, scene[6]["default"], scene[2], "sgm")
    check_ok_lines(r, SELF_CHECKS if host_compare else {k: 0 for k in SELF_CHECKS})


def test_main_sgm_reference_cost(orc, main_cases, scenes, tmp_path):
    scene = scenes["main"]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm", "--cost", "reference", "--sgm-p", "5,40",
                                                 "--sgm-paths", "4", "--host-compare"])
    check_all(orc, files, scene[6]["reference"], scene[2], "sgm on the reference cost")
    check_ok_lines(r, SELF_CHECKS)


def test_main_sgm_census_options_speckle_subpixel(orc, main_cases, scenes, tmp_path):
    scene = scenes["main"]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm", "--census-window", "5x3", "--census-th", "9",
                                                 "--speckle", "30,1", "--subpixel", "parabola", "--host-compare"])
    check_all(orc, files, scene[6]["spk_sub"], scene[2], "sgm speckle subpixel")
    check_ok_lines(r, SELF_CHECKS)


@pytest.mark.parametrize("flags,key,lines", [
    (["--speckle", "30", "--wmf", "occluded"], "spk_wmf", {}),
    (["--wmf", "all", "--host-compare"], "wmf_all", dict(SELF_CHECKS, **{"Weighted median ok!": 1}))],
    ids=["speckle_wmf_occluded", "wmf_all_host_compare"])
def test_main_sgm_weighted_median(orc, main_cases, scenes, tmp_path, flags, key, lines):
    scene = scenes["main"]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm"] + flags)
    check_all(orc, files, scene[6][key], scene[2], "sgm " + " ".join(flags))
    check_ok_lines(r, lines)


def test_main_sgm_pairs_on_one_context(orc, main_cases, scenes, tmp_path):
    """--pairs 3: the context's SGM volumes and workspace are used three times; the files are those of one pair."""
    scene = scenes["main"]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm", "--pairs", "3"])
    assert "pairs 2 on one context" in r.stdout and "(pipelined entry)" not in r.stdout, r.stdout
    check_all(orc, files, scene[6]["default"], scene[2], "sgm pairs 3")


@pytest.mark.parametrize("name", ["x0", "d256"])
def test_main_sgm_other_ranges(orc, main_cases, scenes, tmp_path, name):
    scene = scenes[name]
    r, files = run(tmp_path, scene, ["--aggregation", "sgm", "--host-compare"])
    check_all(orc, files, scene[6]["default"], scene[2], "sgm " + name)
    check_ok_lines(r, SELF_CHECKS)


def test_main_aggregation_guided_is_the_default(main_cases, scenes, tmp_path):
    """--aggregation guided: every file byte for byte what a run without the option writes."""
    left, right, _, _, d_lo, d_hi, _ = scenes["main"]
    plain = assert_same_files_as_plain(tmp_path, left, right, [d_lo, d_hi], ["--aggregation", "guided"])
    assert np.asarray(Image.open(plain / "out" / "image_mean_left.png")).any()


# ---- runs that must be refused -------------------------------------------------------------------------------------------
REFUSED = {
    "sgm_p_without_sgm": (["--sgm-p", "5,40"], None),
    "sgm_paths_with_guided": (["--aggregation", "guided", "--sgm-paths", "4"], None),
    "p1_above_p2": (["--aggregation", "sgm", "--sgm-p", "11,10"], None),
    "p2_above_4095": (["--aggregation", "sgm", "--sgm-p", "1,4096"], None),
    "one_penalty": (["--aggregation", "sgm", "--sgm-p", "7"], None),
    "trailing_text": (["--aggregation", "sgm", "--sgm-p", "1,2x"], None),
    "six_paths": (["--aggregation", "sgm", "--sgm-paths", "6"], None),
    "unknown_aggregation": (["--aggregation", "semi"], None),
    "ngpu": (["--aggregation", "sgm", "--ngpu", "1"], None),
    "pipeline": (["--aggregation", "sgm", "--fused", "--pairs", "3", "--pipeline"], None),
    "257_labels": (["--aggregation", "sgm"], (-256, 0)),
    # (the census options go with the census cost that SGM implies, not with an explicit --cost reference)
    "census_window_on_reference_cost": (["--aggregation", "sgm", "--cost", "reference", "--census-window", "5x3"], None),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_sgm_refuses(main_cases, scenes, tmp_path, case):
    flags, rng = REFUSED[case]
    left, right = scenes["x0"][:2]
    assert_refused(tmp_path, left, right, list(rng or (-5, 6)), flags, ("--aggregation", "--sgm"))


def test_main_refuses_aggregation_without_a_value(main_cases, scenes, tmp_path):
    left, right = scenes["x0"][:2]
    L, R = write_png(tmp_path / "left.png", left), write_png(tmp_path / "right.png", right)
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([build_main(), L, R, "-5", "6", str(out), "--aggregation"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "--aggregation needs a value" in r.stderr, (r.returncode, r.stdout + r.stderr)
    assert not os.listdir(out)
