"""The drop-in main with the scan-line optimiser (`smx_main L R DMIN DMAX OUTDIR --aggregation scanline | cross-scanline
[--so-p P1,P2] [--so-tau T] [--so-paths 4|8]`): every file it writes against a chain of references alone -- the oracle's gray
conversion and cost volume, tests/census_ref.py or tests/adcensus_ref.py, tests/cross_ref.py and tests/scanline_ref.py with the
colour pair as the guide, the oracle's LR check, tests/uniq_ref.py, tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py
/ tests/wmf_ref.py.  With --host-compare the run also executes scanline_optimizeOnCPU (host/cpu_twins.cpp, held to
scanline_ref on the CPU by tests/test_host_scanline_cpu.py) behind cross_aggregateOnCPU, and the check_errors wiring of
host/main.cpp around them.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_scanline
"""
import numpy as np
import pytest

import adcensus_ref
import census_ref
import cgf_ref
import cross_ref
import scanline_ref
import subpix_ref
from main_harness import (assert_refused, assert_same_files_as_plain, check_ok_lines, check_outputs, finish_chain, main_cases,  # noqa: F401
                          run_ok)

pytestmark = pytest.mark.gpu

SPK = (30, 1.0)
PCT = 5.0                                   # --uniqueness PCT
W, H, D_LO, D_HI = 97, 41, -11, 0
CROSS = dict(l1=17, l2=8, tau1=25, tau2=8, iterations=2)
CROSS_FLAGS = ["--cross-arms", "17,8", "--cross-tau", "25,8", "--cross-iterations", "2"]
SO = dict(p1=40, p2=400, tau_so=12, paths=8)
SO_FLAGS = ["--so-p", "40,400", "--so-tau", "12", "--so-paths", "8"]


def chain(orc, left, right, d_lo, d_hi, agg, cost="reference", cross=None, so=None, uniqueness=None, speckle=None, subpixel=None,
          wmf=None):
    """What smx_main --aggregation scanline / cross-scanline computes, from the references alone: {key: array}, the keys of PNGS
    of tests/main_harness.py plus unique / despeckled / sub_filled / refined / final where the options ask for them."""
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    gl, gr = orc.gray(left), orc.gray(right)
    build = {"census": lambda a, b, dm: census_ref.census_cost(a, b, D, dm),
             "adcensus": lambda a, b, dm: adcensus_ref.gray_cost(a, b, D, dm),
             "reference": lambda a, b, dm: orc.cost_volume(a, b, D, dm)}[cost]
    vols = [build(a, b, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    rgb = (left, right)
    states = []
    for v in (0, 1):
        vol = cross_ref.aggregate(rgb[v], vols[v], **(cross or cross_ref.DEFAULTS)) if agg == "cross-scanline" else vols[v]
        S = scanline_ref.aggregate(rgb[v], rgb[1 - v], vol, dmin[v], **(so or scanline_ref.DEFAULTS))
        states.append(cgf_ref.states(S.astype(np.float32)))
    sl, sr = states
    e = {"grayl": gl, "grayr": gr, "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr),      # no mean images
         "cost0l": vols[0][0].copy(), "cost0r": vols[1][0].copy(), "bestl": sl["best"], "bestr": sr["best"],
         "dmapl": subpix_ref.dmap_of(sl["z"], sl["best"], dmin[0]), "dmapr": subpix_ref.dmap_of(sr["z"], sr["best"], dmin[1])}
    return finish_chain(orc, e, d_lo, D, z=sl["z"], best=sl["best"], sec=sl["uq"][0], nbr=sl["nbr"], uniqueness=uniqueness,
                        speckle=speckle, subpixel=subpixel, wmf=wmf)


@pytest.fixture(scope="module")
def scene(orc):
    left, right = cgf_ref.colour_pair(W, H, D_HI - D_LO + 1, 815)
    e = {(agg, "default"): chain(orc, left, right, D_LO, D_HI, agg) for agg in ("scanline", "cross-scanline")}
    for d in e.values():
        assert len(np.unique(d["dmapl"])) >= 2 and len(np.unique(d["dmapr"])) >= 2
    assert np.any(e[("scanline", "default")]["bestl"] != e[("cross-scanline", "default")]["bestl"])
    e[("cross-scanline", "options")] = chain(orc, left, right, D_LO, D_HI, "cross-scanline", cost="adcensus", cross=CROSS, so=SO,
                                             uniqueness=PCT, speckle=SPK, subpixel="parabola")
    e[("scanline", "options")] = chain(orc, left, right, D_LO, D_HI, "scanline", cost="census", so=SO, wmf="occluded")
    plain = chain(orc, left, right, D_LO, D_HI, "scanline", cost="census")
    assert np.any(e[("scanline", "options")]["bestl"] != plain["bestl"])             # the options do something
    return left, right, e


def run(tmp_path, scene, agg, flags, left=None, right=None):
    return run_ok(tmp_path, scene[0] if left is None else left, scene[1] if right is None else right, [D_LO, D_HI],
                  ["--aggregation", agg] + flags)


def check_all(orc, files, e, what):
    check_outputs(orc, files, e, W, H, what, mean_empty=True)


SELF_CHECKS = {"Grayscale ok!": 2, "Scan-line optimisation ok!": 1, "Occlusion ok!": 1}


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
@pytest.mark.parametrize("agg", ["scanline", "cross-scanline"])
def test_main_scanline_defaults(orc, main_cases, scene, tmp_path, agg, host_compare):
    r, files = run(tmp_path, scene, agg, ["--host-compare"] if host_compare else [])
    check_all(orc, files, scene[2][(agg, "default")], agg)
    check_ok_lines(r, {line: count if host_compare else 0 for line, count in SELF_CHECKS.items()})
    assert "Cross-based aggregation ok!" not in r.stdout


def test_main_scanline_four_channels(orc, main_cases, scene, tmp_path):
    rgba = [np.concatenate((x, np.full((H, W, 1), 200, np.uint8)), axis=2) for x in scene[:2]]
    r, files = run(tmp_path, scene, "scanline", [], *rgba)
    check_all(orc, files, scene[2][("scanline", "default")], "scanline rgba")


def test_main_chain_every_option_with_adcensus_uniqueness_speckle_subpixel(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, "cross-scanline", CROSS_FLAGS + SO_FLAGS + ["--cost", "adcensus", "--uniqueness", str(PCT),
                                                                                 "--speckle", "30,1", "--subpixel", "parabola",
                                                                                 "--host-compare"])
    check_all(orc, files, scene[2][("cross-scanline", "options")], "chain options adcensus uniqueness speckle subpixel")
    check_ok_lines(r, dict(SELF_CHECKS, **{"Uniqueness ok!": 1}))


def test_main_scanline_every_option_census_wmf_pairs(orc, main_cases, scene, tmp_path):
    r, files = run(tmp_path, scene, "scanline", SO_FLAGS + ["--cost", "census", "--wmf", "occluded", "--pairs", "2"])
    assert "pairs 1 on one context" in r.stdout
    check_all(orc, files, scene[2][("scanline", "options")], "scanline census wmf")


def test_main_without_the_options_is_unchanged(main_cases, scene, tmp_path):
    """--aggregation guided: the twelve images, the pfm and the png16 byte for byte what a run without the option writes."""
    assert_same_files_as_plain(tmp_path, scene[0], scene[1], [D_LO, D_HI], ["--aggregation", "guided"])


X, Y = ["--aggregation", "scanline"], ["--aggregation", "cross-scanline"]
REFUSED = {   # flags, the label range (None: the scene's) -> the option stderr names
    "guidance_rgb": (X + ["--guidance", "rgb"], None, "--aggregation scanline"),
    "chain_guidance_rgb": (Y + ["--guidance", "rgb"], None, "--aggregation cross-scanline"),
    "ngpu": (X + ["--ngpu", "1"], None, "--aggregation scanline"),
    "pipeline": (Y + ["--fused", "--pairs", "3", "--pipeline"], None, "--aggregation cross-scanline"),
    "257_labels": (X, (-256, 0), "--aggregation scanline"),
    "chain_257_labels": (Y, (-256, 0), "--aggregation cross-scanline"),
    "unknown_aggregation": (["--aggregation", "scan-line"], None, "--aggregation"),
    "p_without_scanline": (["--so-p", "40,400"], None, "--so-p"),
    "tau_with_cross": (["--aggregation", "cross", "--so-tau", "15"], None, "--so-tau"),
    "paths_with_sgm": (["--aggregation", "sgm", "--so-paths", "8"], None, "--so-paths"),
    "sgm_p_with_scanline": (X + ["--sgm-p", "5,40"], None, "--sgm-p"),
    "cross_arms_with_scanline": (X + ["--cross-arms", "17,8"], None, "--cross-arms"),
    "p1_above_p2": (X + ["--so-p", "11,10"], None, "--so-p"),
    "p2_above_4095": (X + ["--so-p", "1,4096"], None, "--so-p"),
    "one_penalty": (X + ["--so-p", "7"], None, "--so-p"),
    "p_trailing_text": (X + ["--so-p", "1,2x"], None, "--so-p"),
    "tau_0": (X + ["--so-tau", "0"], None, "--so-tau"),
    "tau_257": (X + ["--so-tau", "257"], None, "--so-tau"),
    "tau_text": (X + ["--so-tau", "15x"], None, "--so-tau"),
    "six_paths": (Y + ["--so-paths", "6"], None, "--so-paths"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_scanline_refuses(main_cases, scene, tmp_path, case):
    flags, rng, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], list(rng or (D_LO, D_HI)), flags, name)
