"""The drop-in main with the colour-guided filter (`smx_main L R DMIN DMAX OUTDIR --guidance rgb ...`): every file it writes
against a chain of references alone -- the oracle's gray conversion and cost volume or tests/census_ref.py, tests/cgf_ref.py,
the oracle's LR check, tests/uniq_ref.py, tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py / tests/wmf_ref.py;
the 8-bit images are oracle.write_mat_u8 of the expected map.  That chain is what PairPipeline(guidance="rgb") is held to in
tests/test_gpu_cgf.py, so the outputs equal the pipeline's.  With --host-compare the run also executes
colour_guided_filterOnCPU (host/cpu_twins.cpp, held to cgf_ref on the CPU by tests/test_cgf_cpu.py) and the check_errors
wiring of host/main.cpp around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_cgf
"""
import numpy as np
import pytest

import census_ref
import cgf_ref
import subpix_ref
from main_harness import (assert_refused, assert_same_files_as_plain, check_ok_lines, check_outputs, finish_chain, main_cases,  # noqa: F401
                          run_ok)

pytestmark = pytest.mark.gpu

SPK = (30, 1.0)
PCT = 13.0                                  # --uniqueness PCT
W, H, D_LO, D_HI = 97, 41, -11, 0


def chain(orc, left, right, d_lo, d_hi, cost="reference", uniqueness=None, speckle=None, subpixel=None, wmf=None):
    """What smx_main --guidance rgb computes, from the references alone: {key: array}, the keys of PNGS of
    tests/main_harness.py plus unique / despeckled / sub_filled / refined / final where the options ask for them."""
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    gl, gr = orc.gray(left), orc.gray(right)
    if cost == "census":
        vols = [census_ref.census_cost(a, b, D, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    else:
        vols = [orc.cost_volume(a, b, D, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    sl, sr = (cgf_ref.outputs(g, v) for g, v in zip((left, right), vols))
    e = {"grayl": gl, "grayr": gr, "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr),      # no mean images
         "cost0l": vols[0][0].copy(), "cost0r": vols[1][0].copy(), "bestl": sl["best"], "bestr": sr["best"],
         "dmapl": subpix_ref.dmap_of(sl["z"], sl["best"], dmin[0]), "dmapr": subpix_ref.dmap_of(sr["z"], sr["best"], dmin[1])}
    return finish_chain(orc, e, d_lo, D, z=sl["z"], best=sl["best"], sec=sl["uq"][0], nbr=sl["nbr"], uniqueness=uniqueness,
                        speckle=speckle, subpixel=subpixel, wmf=wmf)


@pytest.fixture(scope="module")
def scene(orc):
    left, right = cgf_ref.colour_pair(W, H, D_HI - D_LO + 1, 815)
    e = {"default": chain(orc, left, right, D_LO, D_HI)}
    d = e["default"]
    dropped = int((d["occlusion"] == D_LO - 100).sum())
    assert 0 < dropped < W * H and np.any(d["filled"] != d["occlusion"])
    assert len(np.unique(d["dmapl"])) >= 2 and len(np.unique(d["dmapr"])) >= 2
    # the colour guide gives another result than the gray one: the test would pass on nothing otherwise
    gray = orc.stereo_pair(d["grayl"], d["grayr"], D_HI - D_LO + 1, dminl=D_LO, dminr=-D_HI)
    assert np.any(gray["bestl"] != d["bestl"])
    e["census_all"] = chain(orc, left, right, D_LO, D_HI, cost="census", uniqueness=PCT, speckle=SPK, subpixel="parabola")
    e["uniq_spk_wmf"] = chain(orc, left, right, D_LO, D_HI, uniqueness=PCT, speckle=SPK, wmf="occluded")
    for k in ("census_all", "uniq_spk_wmf"):
        assert np.any(e[k]["unique"] != e[k]["occlusion"]), k
        assert np.any(e[k]["despeckled"] != e[k]["unique"]), k
    assert np.any(e["census_all"]["sub_filled"] != np.trunc(e["census_all"]["sub_filled"]))
    assert np.any(e["uniq_spk_wmf"]["refined"] != e["uniq_spk_wmf"]["filled"])
    return left, right, e


def run(tmp_path, scene, flags, left=None, right=None):
    return run_ok(tmp_path, scene[0] if left is None else left, scene[1] if right is None else right, [D_LO, D_HI],
                  ["--guidance", "rgb"] + flags)


def check_all(orc, files, e, what):
    check_outputs(orc, files, e, W, H, what, mean_empty=True)


SELF_CHECKS = {"Grayscale ok!": 2, "Colour guided filter ok!": 1, "Occlusion ok!": 1}


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_cgf_defaults(orc, main_cases, scene, tmp_path, host_compare):
    r, files = run(tmp_path, scene, ["--host-compare"] if host_compare else [])
    check_all(orc, files, scene[2]["default"], "cgf")
    check_ok_lines(r, {line: count if host_compare else 0 for line, count in SELF_CHECKS.items()})


def test_main_cgf_four_channels(orc, main_cases, scene, tmp_path):
    rgba = [np.concatenate((x, np.full((H, W, 1), 200, np.uint8)), axis=2) for x in scene[:2]]
    r, files = run(tmp_path, scene, [], *rgba)
    check_all(orc, files, scene[2]["default"], "cgf rgba")


def test_main_cgf_census_uniqueness_speckle_subpixel(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, ["--cost", "census", "--uniqueness", str(PCT), "--speckle", "30,1", "--subpixel",
                                                 "parabola", "--host-compare"])
    check_all(orc, files, scene[2]["census_all"], "cgf census uniqueness speckle subpixel")
    check_ok_lines(r, dict(SELF_CHECKS, **{"Uniqueness ok!": 1}))


def test_main_cgf_uniqueness_speckle_wmf_pairs(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, ["--uniqueness", str(PCT), "--speckle", "30", "--wmf", "occluded", "--pairs", "2"])
    assert "pairs 1 on one context" in r.stdout
    check_all(orc, files, scene[2]["uniq_spk_wmf"], "cgf uniqueness speckle wmf")


def test_main_guidance_gray_is_the_default(main_cases, scene, tmp_path):
    """--guidance gray: every file byte for byte what a run without the option writes."""
    assert_same_files_as_plain(tmp_path, scene[0], scene[1], [D_LO, D_HI], ["--guidance", "gray"])


REFUSED = {
    "sgm": ["--guidance", "rgb", "--aggregation", "sgm"],
    "ngpu": ["--guidance", "rgb", "--ngpu", "1"],
    "pipeline": ["--guidance", "rgb", "--fused", "--pairs", "3", "--pipeline"],
    "unknown_guide": ["--guidance", "colour"],
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_cgf_refuses(main_cases, scene, tmp_path, case):
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], REFUSED[case], "--guidance")
