"""The drop-in main with region voting (`smx_main L R DMIN DMAX OUTDIR --vote [S,PCT[,N]] [--vote-interpolate 0|1] [--vote-arms
L1,L2] [--vote-tau T1,T2]`): every file it writes against a chain of references alone -- the oracle's pair or the chain of
tests/test_gpu_main_cross.py up to the winners, then tests/vote_ref.py's chain.  With --host-compare the run also executes
region_voteOnCPU (host/cpu_twins.cpp, held to vote_ref on the CPU by tests/test_host_vote_cpu.py) and the check_errors wiring of
host/main.cpp around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_vote
"""
import numpy as np
import pytest

import adcensus_ref
import cgf_ref
import cross_ref
import main_harness
import vote_ref
from main_harness import (OPTIONAL_PNGS, assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits)  # noqa: F401
from test_gpu_main_cross import chain as cross_chain

pytestmark = pytest.mark.gpu

W, H, D_LO, D_HI = 97, 41, -11, 0
D = D_HI - D_LO + 1
SPK = (30, 1.0)
PCT = 4.0
CROSS = dict(l1=17, l2=8, tau1=25, tau2=8, iterations=2)
CROSS_FLAGS = ["--aggregation", "cross", "--cross-arms", "17,8", "--cross-tau", "25,8", "--cross-iterations", "2"]
OPTIONS = dict(tau_s=5, tau_h_pct=30, iterations=3, interpolate_=0)
OPTION_ARMS = dict(l1=9, l2=4, tau1=30, tau2=10)
OPTION_FLAGS = ["--vote", "5,30,3", "--vote-interpolate", "0", "--vote-arms", "9,4", "--vote-tau", "30,10"]


def guided_winners(orc, gl, gr):
    w = orc.stereo_pair(gl, gr, D, dminl=D_LO, dminr=-D_HI, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy()}
    e.update({k: w[k] for k in ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr")})
    return e, cgf_ref.states(w["aggl"])


@pytest.fixture(scope="module")
def scene(orc):
    left, right = cgf_ref.colour_pair(W, H, D, 815)
    return left, right, orc.gray(left), orc.gray(right)


def with_vote(orc, e, sl, guide, vote, arms=None, **stages):
    return vote_ref.chain(orc, e, D_LO, D, guide, vote, arms, 0, z=sl["z"], best=sl["best"], sec=sl["uq"][0], nbr=sl["nbr"], **stages)


def check_all(orc, files, e, what, mean_empty=False):
    check_outputs(orc, files, e, W, H, what, mean_empty=mean_empty)
    same_bits(files["png"]["occlu_mapl_voted"], orc.write_mat_u8(e["voted"]), what + " occlu_mapl_voted.png")
    kept = e.get("despeckled", e.get("unique", e["occlusion"]))
    assert np.any(e["voted"] != kept), what + ": the stage changed nothing on the reference values"
    assert "occlu_mapl_voted" not in OPTIONAL_PNGS


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
@pytest.mark.parametrize("fused", [False, True], ids=["stages", "fused"])
def test_main_vote_defaults(orc, main_cases, scene, tmp_path, fused, host_compare):
    """the reference's flow stage by stage and the device-resident one: the guide is the gray left image in both"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], (["--fused"] if fused else []) + ["--vote"] +
                      (["--host-compare"] if host_compare else []))
    e, sl = guided_winners(orc, gl, gr)
    check_all(orc, files, with_vote(orc, e, sl, gl, {}), "defaults")
    check_ok_lines(r, {"Region voting ok!": int(host_compare)})


def test_main_vote_every_option_behind_cross_adcensus_uniqueness_speckle_subpixel(orc, main_cases, scene, tmp_path):
    """the colour entry: the guide of the vote is the left colour image"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], CROSS_FLAGS + OPTION_FLAGS + [
        "--cost", "adcensus", "--uniqueness", str(PCT), "--speckle", "30,1", "--subpixel", "parabola", "--host-compare"])
    e = cross_chain(orc, left, right, D_LO, D_HI, cost="adcensus", params=CROSS)
    sl = cgf_ref.states(cross_ref.aggregate(left, adcensus_ref.gray_cost(gl, gr, D, D_LO), **CROSS))
    e = with_vote(orc, e, sl, left, OPTIONS, OPTION_ARMS, uniqueness=PCT, speckle=SPK, subpixel="parabola")
    check_all(orc, files, e, "every option", mean_empty=True)
    check_ok_lines(r, {"Region voting ok!": 1, "Uniqueness ok!": 1, "Occlusion ok!": 1, "Cross-based aggregation ok!": 1})


def test_main_vote_two_values_fused_wmf(orc, main_cases, scene, tmp_path):
    """S,PCT without N keeps the default number of rounds; --wmf occluded refines the pixels the LR check invalidated"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--fused", "--vote", "3,20", "--wmf", "occluded", "--pairs", "2"])
    e, sl = guided_winners(orc, gl, gr)
    check_all(orc, files, with_vote(orc, e, sl, gl, dict(tau_s=3, tau_h_pct=20), wmf="occluded"), "two values")


def test_main_without_vote_writes_what_it_wrote(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], [])
    e, sl = guided_winners(orc, gl, gr)
    check_outputs(orc, files, main_harness.finish_chain(orc, e, D_LO, D), W, H, "no --vote")
    assert "occlu_mapl_voted" not in files["png"] and len(files["png"]) == 12


V = ["--vote"]
REFUSED = {   # flags -> the option stderr names
    "ngpu": (V + ["--ngpu", "1"], "--vote"),
    "pipeline": (V + ["--fused", "--pairs", "3", "--pipeline"], "--vote"),
    "arms_without_vote": (["--vote-arms", "17,8"], "--vote-arms"),
    "tau_without_vote": (["--vote-tau", "20,6"], "--vote-tau"),
    "interpolate_without_vote": (["--vote-interpolate", "1"], "--vote-interpolate"),
    "one_value": (["--vote", "5"], "--vote"),
    "pct_100": (["--vote", "5,100"], "--vote"),
    "rounds_9": (["--vote", "5,30,9"], "--vote"),
    "four_values": (["--vote", "5,30,3,1"], "--vote"),
    "trailing_text": (["--vote", "5,30x"], "--vote"),
    "interpolate_2": (V + ["--vote-interpolate", "2"], "--vote-interpolate"),
    "l1_64": (V + ["--vote-arms", "64,1"], "--vote-arms"),
    "l2_above_l1": (V + ["--vote-arms", "5,6"], "--vote-arms"),
    "tau2_above_tau1": (V + ["--vote-tau", "6,20"], "--vote-tau"),
    "tau1_257": (V + ["--vote-tau", "257,6"], "--vote-tau"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_vote_refuses(main_cases, scene, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], flags, name)


def test_main_vote_refuses_more_than_512_labels(main_cases, scene, tmp_path):
    assert_refused(tmp_path, scene[0], scene[1], [-512, 0], V, "--vote")
