"""The drop-in main with belief propagation (`smx_main L R DMIN DMAX OUTDIR --aggregation bp [--bp-*]`) on the Tsukuba fixture and
on the 64 x 9 pair of a recorded case of the reference: every file it writes against references alone -- the oracle's cost
volumes, tests/bp_ref.py, tests/main_harness.py's chain behind the winners.  With --host-compare the run also executes the
twins (the cost twins, beliefPropagationOnCPU; the last held to bp_ref on the CPU by tests/test_host_bp_cpu.py) and must print
"Belief propagation ok!".

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_bp
"""
import numpy as np
import pytest

import bp_ref as ref
import main_harness
import ref_fixtures as rf
from main_harness import assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32
SMALL = "cli_one_64x9"          # (its images; the recorded range has one label, so the tests give their own)
D_LO, D_HI = -8, 0


def expected(orc, left, right, d_lo, d_hi, params=(20, 60, 5, 4, 1.0), **later):
    """the maps of a pair with belief propagation on the reference's cost: the mean images are empty"""
    D = d_hi - d_lo + 1
    gl, gr = orc.gray(left), orc.gray(right)
    cl, cr = orc.cost_volume(gl, gr, D, d_lo), orc.cost_volume(gr, gl, D, -d_hi)
    e = {"grayl": gl, "grayr": gr, "cost0l": cl[0].copy(), "cost0r": cr[0].copy(), "meanl": np.zeros_like(gl),
         "meanr": np.zeros_like(gr)}
    out = {}
    for side, cost, dmin in (("l", cl, d_lo), ("r", cr, -d_hi)):
        out[side] = o = ref.outputs(cost, *params)
        e["dmap" + side] = (dmin + o["z"]).astype(F32)
        e["best" + side] = o["best"]
    o = out["l"]
    return main_harness.finish_chain(orc, e, d_lo, D, z=o["z"], best=o["best"], sec=o["uq"][0], nbr=o["nbr"], **later)


@pytest.fixture(scope="module")
def small():
    c, _ = rf.load(SMALL)
    inp = rf.inputs(c)
    assert (c["w"], c["h"]) == (64, 9)
    return inp["left"], inp["right"]


def test_main_bp_on_tsukuba_with_host_compare(orc, main_cases, golden, tmp_path):
    left, right = golden["tsukuba0"], golden["tsukuba1"]
    h, w = left.shape[:2]
    flags = ["--aggregation", "bp", "--bp-scale", "16", "--host-compare"]
    r, files = run_ok(tmp_path, left, right, [-15, 0], flags)
    e = expected(orc, left, right, -15, 0, (20, 60, 5, 4, 16.0))
    check_outputs(orc, files, e, w, h, "tsukuba --aggregation bp", mean_empty=True)
    same_bits(files["png"]["disparity_mapl_bp"], orc.write_mat_u8(e["dmapl"]), "disparity_mapl_bp.png")
    check_ok_lines(r, {"Belief propagation ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13


@pytest.mark.parametrize("flags,params", [([], (20, 60, 5, 4, 1.0)),
                                          (["--bp-step", "3", "--bp-trunc", "9", "--bp-iterations", "2", "--bp-levels", "2", "--bp-scale",
                                            "24.5"], (3, 9, 2, 2, 24.5))], ids=["defaults", "every_option"])
def test_main_bp_on_a_recorded_pair(orc, main_cases, small, tmp_path, flags, params):
    left, right = small
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--aggregation", "bp", "--host-compare"] + flags)
    e = expected(orc, left, right, D_LO, D_HI, params)
    check_outputs(orc, files, e, 64, 9, " ".join(flags), mean_empty=True)
    same_bits(files["png"]["disparity_mapl_bp"], orc.write_mat_u8(e["dmapl"]), "disparity_mapl_bp.png")
    check_ok_lines(r, {"Belief propagation ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13


def test_main_bp_without_host_compare_and_with_the_later_stages(orc, main_cases, small, tmp_path):
    left, right = small
    flags = ["--aggregation", "bp", "--bp-scale", "16", "--uniqueness", "10", "--speckle", "30,1", "--subpixel", "parabola"]
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], flags)
    e = expected(orc, left, right, D_LO, D_HI, (20, 60, 5, 4, 16.0), uniqueness=10, speckle=(30, 1.0), subpixel="parabola")
    check_outputs(orc, files, e, 64, 9, " ".join(flags), mean_empty=True)
    check_ok_lines(r, {"Belief propagation ok!": 0})


@pytest.mark.parametrize("flags", [["--cost", "census"], ["--cost", "adcensus", "--ad", "rgb"],
                                   ["--cost", "census", "--uniqueness", "4", "--adjust", "--subpixel", "equiangular"]],
                         ids=["census", "adcensus_rgb", "census_uniqueness_adjust_subpixel"])
def test_main_bp_twin_agrees_under_the_other_costs(main_cases, small, tmp_path, flags):
    left, right = small
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--aggregation", "bp", "--host-compare"] + flags)
    check_ok_lines(r, {"Belief propagation ok!": 1, "Occlusion ok!": 1})
    assert "disparity_mapl_bp" in files["png"] and not files["png"]["image_mean_left"].any()


def test_main_without_bp_writes_no_such_map(main_cases, small, tmp_path):
    left, right = small
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--fused"])
    assert "disparity_mapl_bp" not in files["png"] and len(files["png"]) == 12


A = ["--aggregation", "bp"]
REFUSED = {   # flags -> the option stderr names
    "rgb": (A + ["--guidance", "rgb"], "--aggregation bp"),
    "cross_scale": (A + ["--cross-scale"], "--aggregation bp"),
    "permeability": (A + ["--permeability"], "--permeability"),
    "ngpu": (A + ["--ngpu", "1"], "--aggregation bp"),
    "pipeline": (A + ["--fused", "--pairs", "3", "--pipeline"], "--aggregation bp"),
    "step": (A + ["--bp-step", "4096"], "--bp-step"),
    "scale_without_bp": (["--bp-scale", "2"], "--bp-scale"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_bp_refuses(main_cases, small, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, small[0], small[1], [D_LO, D_HI], flags, name)


def test_main_bp_refuses_more_than_256_labels(main_cases, small, tmp_path):
    assert_refused(tmp_path, small[0], small[1], [-256, 0], A, "--aggregation bp takes at most 256 labels")
