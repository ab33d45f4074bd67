"""The drop-in main with the depth-discontinuity adjustment (`smx_main L R DMIN DMAX OUTDIR --adjust [TAU[,N]] [--adjust-vertical
0|1]`): every file it writes against a chain of references alone -- the oracle's pair or the chain of
tests/test_gpu_main_cross.py up to the winners, tests/main_harness.py's / tests/vote_ref.py's chain up to the sub-pixel fit, then
tests/adjust_ref.py on the left aggregated volume.  With --host-compare the run also executes discontinuityAdjustOnCPU
(host/cpu_twins.cpp, held to adjust_ref on the CPU by tests/test_host_adjust_cpu.py) and the check_errors wiring of host/main.cpp
around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_adjust
"""
import numpy as np
import pytest

import adcensus_ref
import adjust_ref
import cgf_ref
import cross_ref
import main_harness
import subpix_ref
import vote_ref
import wmf_ref
from main_harness import (OPTIONAL_PNGS, assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits)  # noqa: F401
from test_gpu_main_cross import chain as cross_chain

pytestmark = pytest.mark.gpu

W, H, D_LO, D_HI = 97, 41, -11, 0
D = D_HI - D_LO + 1
SPK = (30, 1.0)
PCT = 4.0
CROSS = dict(l1=17, l2=8, tau1=25, tau2=8, iterations=2)
CROSS_FLAGS = ["--aggregation", "cross", "--cross-arms", "17,8", "--cross-tau", "25,8", "--cross-iterations", "2"]
VOTE = dict(tau_s=5, tau_h_pct=30, iterations=3, interpolate_=1)
VOTE_ARMS = dict(l1=9, l2=4, tau1=30, tau2=10)
VOTE_FLAGS = ["--vote", "5,30,3", "--vote-arms", "9,4", "--vote-tau", "30,10"]
OPTIONS = dict(tau_e=1, vertical=0, iterations=3)
OPTION_FLAGS = ["--adjust", "1,3", "--adjust-vertical", "0"]


def guided_winners(orc, gl, gr):
    w = orc.stereo_pair(gl, gr, D, dminl=D_LO, dminr=-D_HI, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy()}
    e.update({k: w[k] for k in ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr")})
    return e, w["aggl"]


@pytest.fixture(scope="module")
def scene(orc):
    left, right = cgf_ref.colour_pair(W, H, D, 815)
    return left, right, orc.gray(left), orc.gray(right)


def with_adjust(orc, e, aggl, adjust, vote=None, subpixel=None, wmf=None, **stages):
    """the chain of the main behind the winners of `aggl`, with the stage in its place: ... -> fill -> sub-pixel fit ->
    adjustment -> weighted median.  vote: None, or (guide, vote, arms)"""
    sl = cgf_ref.states(aggl)
    kw = dict(z=sl["z"], best=sl["best"], sec=sl["uq"][0], nbr=sl["nbr"], subpixel=subpixel, **stages)
    if vote is not None:
        vote_ref.chain(orc, e, D_LO, D, vote[0], vote[1], vote[2], 0, **kw)
    else:
        main_harness.finish_chain(orc, e, D_LO, D, **kw)
    e["before"] = e["filled"]
    if subpixel:
        e["filled"], e["sub_filled"] = adjust_ref.adjust(e["before"], aggl, D_LO, mode=subpix_ref.MODES[subpixel], sub=e["sub_filled"],
                                                         **adjust)
        e["final"] = e["sub_filled"]
    else:
        e["filled"] = e["final"] = adjust_ref.adjust(e["before"], aggl, D_LO, **adjust)
    if wmf:
        kept = e.get("despeckled", e.get("unique", e["occlusion"]))
        e["refined"] = e["final"] = wmf_ref.weighted_median(e["grayl"], e["filled"], D_LO, D, kept if wmf == "occluded" else None)
    return e


def check_all(orc, files, e, what, mean_empty=False):
    check_outputs(orc, files, e, W, H, what, mean_empty=mean_empty)
    same_bits(files["png"]["occlu_mapl_adjusted"], orc.write_mat_u8(e["filled"]), what + " occlu_mapl_adjusted.png")
    if "voted" in e:
        same_bits(files["png"]["occlu_mapl_voted"], orc.write_mat_u8(e["voted"]), what + " occlu_mapl_voted.png")
    assert np.any(e["filled"] != e["before"]), what + ": the stage changed nothing on the reference values"
    assert "occlu_mapl_adjusted" not in OPTIONAL_PNGS


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_adjust_defaults(orc, main_cases, scene, tmp_path, host_compare):
    """--adjust alone implies the device-resident flow: the stage needs the aggregated volume"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--adjust"] + (["--host-compare"] if host_compare else []))
    e, aggl = guided_winners(orc, gl, gr)
    check_all(orc, files, with_adjust(orc, e, aggl, adjust_ref.DEFAULTS), "defaults")
    check_ok_lines(r, {"Discontinuity adjustment ok!": int(host_compare), "Occlusion ok!": int(host_compare)})
    assert len(files["png"]) == 13


def test_main_adjust_every_option_behind_cross_adcensus_uniqueness_speckle_vote_subpixel(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], CROSS_FLAGS + OPTION_FLAGS + VOTE_FLAGS + [
        "--cost", "adcensus", "--uniqueness", str(PCT), "--speckle", "30,1", "--subpixel", "equiangular", "--host-compare"])
    e = cross_chain(orc, left, right, D_LO, D_HI, cost="adcensus", params=CROSS)
    aggl = cross_ref.aggregate(left, adcensus_ref.gray_cost(gl, gr, D, D_LO), **CROSS)
    e = with_adjust(orc, e, aggl, OPTIONS, vote=(left, VOTE, VOTE_ARMS), uniqueness=PCT, speckle=SPK, subpixel="equiangular")
    check_all(orc, files, e, "every option", mean_empty=True)
    check_ok_lines(r, {"Discontinuity adjustment ok!": 1, "Region voting ok!": 1, "Uniqueness ok!": 1, "Occlusion ok!": 1,
                       "Cross-based aggregation ok!": 1})
    assert np.any(e["sub_filled"] != e["filled"])


def test_main_adjust_one_value_wmf_and_pairs(orc, main_cases, scene, tmp_path):
    """TAU without N keeps the default single round; --wmf refines the adjusted map"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--adjust", "1", "--wmf", "occluded", "--pairs", "2"])
    e, aggl = guided_winners(orc, gl, gr)
    check_all(orc, files, with_adjust(orc, e, aggl, dict(tau_e=1, vertical=1, iterations=1), wmf="occluded"), "one value")


def test_main_without_adjust_writes_what_it_wrote(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], [])
    e, _ = guided_winners(orc, gl, gr)
    check_outputs(orc, files, main_harness.finish_chain(orc, e, D_LO, D), W, H, "no --adjust")
    assert "occlu_mapl_adjusted" not in files["png"] and len(files["png"]) == 12


A = ["--adjust"]
REFUSED = {   # flags -> the option stderr names
    "ngpu": (A + ["--ngpu", "1"], "--adjust"),
    "pipeline": (A + ["--fused", "--pairs", "3", "--pipeline"], "--adjust"),
    "vertical_without_adjust": (["--adjust-vertical", "1"], "--adjust-vertical"),
    "tau_0": (["--adjust", "0"], "--adjust"),
    "tau_513": (["--adjust", "513"], "--adjust"),
    "rounds_0": (["--adjust", "2,0"], "--adjust"),
    "rounds_9": (["--adjust", "2,9"], "--adjust"),
    "three_values": (["--adjust", "2,1,1"], "--adjust"),
    "trailing_text": (["--adjust", "2x"], "--adjust"),
    "vertical_2": (A + ["--adjust-vertical", "2"], "--adjust-vertical"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_adjust_refuses(main_cases, scene, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], flags, name)


def test_main_adjust_refuses_more_than_512_labels(main_cases, scene, tmp_path):
    assert_refused(tmp_path, scene[0], scene[1], [-512, 0], A, "--adjust")
