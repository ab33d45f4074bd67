"""The drop-in main with cross-based aggregation (`smx_main L R DMIN DMAX OUTDIR --aggregation cross [--cross-arms L1,L2]
[--cross-tau T1,T2] [--cross-iterations N]`): every file it writes against a chain of references alone -- the oracle's gray
conversion and cost volume, tests/census_ref.py or tests/adcensus_ref.py, tests/cross_ref.py with the colour pair as the guide,
the oracle's LR check, tests/uniq_ref.py, tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py / tests/wmf_ref.py.
With --host-compare the run also executes cross_aggregateOnCPU (host/cpu_twins.cpp, held to cross_ref on the CPU by
tests/test_host_cross_cpu.py) and the check_errors wiring of host/main.cpp around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_cross
"""
import numpy as np
import pytest

import adcensus_ref
import census_ref
import cgf_ref
import cross_ref
import subpix_ref
from main_harness import (assert_refused, assert_same_files_as_plain, check_ok_lines, check_outputs, finish_chain, main_cases,  # noqa: F401
                          run_ok)

pytestmark = pytest.mark.gpu

SPK = (30, 1.0)
PCT = 13.0                                  # --uniqueness PCT
W, H, D_LO, D_HI = 97, 41, -11, 0
OPTIONS = dict(l1=17, l2=8, tau1=25, tau2=8, iterations=2)
OPTION_FLAGS = ["--cross-arms", "17,8", "--cross-tau", "25,8", "--cross-iterations", "2"]


def chain(orc, left, right, d_lo, d_hi, cost="reference", params=None, uniqueness=None, speckle=None, subpixel=None, wmf=None):
    """What smx_main --aggregation cross computes, from the references alone: {key: array}, the keys of PNGS of
    tests/main_harness.py plus unique / despeckled / sub_filled / refined / final where the options ask for them."""
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    gl, gr = orc.gray(left), orc.gray(right)
    build = {"census": lambda a, b, dm: census_ref.census_cost(a, b, D, dm),
             "adcensus": lambda a, b, dm: adcensus_ref.gray_cost(a, b, D, dm),
             "reference": lambda a, b, dm: orc.cost_volume(a, b, D, dm)}[cost]
    vols = [build(a, b, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    sl, sr = (cgf_ref.states(cross_ref.aggregate(g, v, **(params or cross_ref.DEFAULTS))) for g, v in zip((left, right), vols))
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
    assert len(np.unique(d["dmapl"])) >= 2 and len(np.unique(d["dmapr"])) >= 2
    # cross-based aggregation gives another result than the guided filter: the test would pass on nothing otherwise
    gray = orc.stereo_pair(d["grayl"], d["grayr"], D_HI - D_LO + 1, dminl=D_LO, dminr=-D_HI)
    assert np.any(gray["bestl"] != d["bestl"])
    e["options"] = chain(orc, left, right, D_LO, D_HI, cost="adcensus", params=OPTIONS, uniqueness=PCT, speckle=SPK,
                         subpixel="parabola")
    e["census_wmf"] = chain(orc, left, right, D_LO, D_HI, cost="census", params=OPTIONS, wmf="occluded")
    assert np.any(e["options"]["bestl"] != chain(orc, left, right, D_LO, D_HI, cost="adcensus")["bestl"])
    return left, right, e


def run(tmp_path, scene, flags, left=None, right=None):
    return run_ok(tmp_path, scene[0] if left is None else left, scene[1] if right is None else right, [D_LO, D_HI],
                  ["--aggregation", "cross"] + flags)


def check_all(orc, files, e, what):
    check_outputs(orc, files, e, W, H, what, mean_empty=True)


SELF_CHECKS = {"Grayscale ok!": 2, "Cross-based aggregation ok!": 1, "Occlusion ok!": 1}


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_cross_defaults(orc, main_cases, scene, tmp_path, host_compare):
    r, files = run(tmp_path, scene, ["--host-compare"] if host_compare else [])
    check_all(orc, files, scene[2]["default"], "cross")
    check_ok_lines(r, {line: count if host_compare else 0 for line, count in SELF_CHECKS.items()})


def test_main_cross_four_channels(orc, main_cases, scene, tmp_path):
    rgba = [np.concatenate((x, np.full((H, W, 1), 200, np.uint8)), axis=2) for x in scene[:2]]
    r, files = run(tmp_path, scene, [], *rgba)
    check_all(orc, files, scene[2]["default"], "cross rgba")


def test_main_cross_every_option_with_adcensus_uniqueness_speckle_subpixel(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, OPTION_FLAGS + ["--cost", "adcensus", "--uniqueness", str(PCT), "--speckle", "30,1",
                                                                "--subpixel", "parabola", "--host-compare"])
    check_all(orc, files, scene[2]["options"], "cross options adcensus uniqueness speckle subpixel")
    check_ok_lines(r, dict(SELF_CHECKS, **{"Uniqueness ok!": 1}))


def test_main_cross_census_wmf_pairs(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, OPTION_FLAGS + ["--cost", "census", "--wmf", "occluded", "--pairs", "2"])
    assert "pairs 1 on one context" in r.stdout
    check_all(orc, files, scene[2]["census_wmf"], "cross census wmf")


def test_main_aggregation_guided_is_the_default(main_cases, scene, tmp_path):
    """--aggregation guided: every file byte for byte what a run without the option writes."""
    assert_same_files_as_plain(tmp_path, scene[0], scene[1], [D_LO, D_HI], ["--aggregation", "guided"])


X = ["--aggregation", "cross"]
REFUSED = {   # flags -> the option stderr names
    "guidance_rgb": (X + ["--guidance", "rgb"], "--aggregation cross"),
    "ngpu": (X + ["--ngpu", "1"], "--aggregation cross"),
    "pipeline": (X + ["--fused", "--pairs", "3", "--pipeline"], "--aggregation cross"),
    "unknown_aggregation": (["--aggregation", "crossed"], "--aggregation"),
    "arms_without_cross": (["--cross-arms", "17,8"], "--cross-arms"),
    "tau_with_guided": (["--aggregation", "guided", "--cross-tau", "20,6"], "--cross-tau"),
    "iterations_with_sgm": (["--aggregation", "sgm", "--cross-iterations", "2"], "--cross-iterations"),
    "l1_64": (X + ["--cross-arms", "64,1"], "--cross-arms"),
    "l1_0": (X + ["--cross-arms", "0,0"], "--cross-arms"),
    "l2_above_l1": (X + ["--cross-arms", "5,6"], "--cross-arms"),
    "one_arm": (X + ["--cross-arms", "17"], "--cross-arms"),
    "arms_trailing_text": (X + ["--cross-arms", "17,8x"], "--cross-arms"),
    "tau2_above_tau1": (X + ["--cross-tau", "6,20"], "--cross-tau"),
    "tau1_257": (X + ["--cross-tau", "257,6"], "--cross-tau"),
    "tau2_0": (X + ["--cross-tau", "20,0"], "--cross-tau"),
    "tau_semicolon": (X + ["--cross-tau", "20;6"], "--cross-tau"),
    "iterations_0": (X + ["--cross-iterations", "0"], "--cross-iterations"),
    "iterations_5": (X + ["--cross-iterations", "5"], "--cross-iterations"),
    "iterations_text": (X + ["--cross-iterations", "two"], "--cross-iterations"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_cross_refuses(main_cases, scene, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], flags, name)
