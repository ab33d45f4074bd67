"""The drop-in main with the permeability filter (`smx_main L R DMIN DMAX OUTDIR --permeability [SIGMA]`) on the Tsukuba fixture
and on a small recorded pair of the reference (cli_19x40): every file it writes against references alone -- the oracle's
aggregated volumes, tests/perm_ref.py's filter and winners, tests/main_harness.py's chain behind them.  With --host-compare the
run also executes the twins (the cost and guided-filter twins, permeabilityOnCPU; the last held to perm_ref on the CPU by
tests/test_host_perm_cpu.py) and must print "Permeability ok!".

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_perm
"""
import numpy as np
import pytest

import main_harness
import perm_ref as ref
import ref_fixtures as rf
import subpix_ref
from main_harness import assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits  # noqa: F401
from oracle import ref_cases as rc

pytestmark = pytest.mark.gpu

F32 = np.float32
PRESET = np.uint32(0x7F7F7F7F).view(F32)
SMALL = "cli_19x40"


def expected(orc, left, right, d_lo, d_hi, sigma, **later):
    """the maps of a pair with the filter behind the guided filter (gray guide): the mean images are empty"""
    D = d_hi - d_lo + 1
    gl, gr = orc.gray(left), orc.gray(right)
    w = orc.stereo_pair(gl, gr, D, dminl=d_lo, dminr=-d_hi, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy(),
         "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr)}
    for side, vol, guide, dmin in (("l", w["aggl"], gl, d_lo), ("r", w["aggr"], gr, -d_hi)):
        z, c0 = ref.winners(ref.filter_volume(vol, guide, sigma))
        e["dmap" + side] = subpix_ref.dmap_of(z, c0, dmin)
        e["best" + side] = np.where((z >= 0) & (PRESET >= c0), c0, PRESET).astype(F32)
    changed = int((e["dmapl"] != w["dmapl"]).sum())
    return main_harness.finish_chain(orc, e, d_lo, D, **later), changed


@pytest.fixture(scope="module")
def small():
    c, _ = rf.load(SMALL)
    inp = rf.inputs(c)
    return inp["left"], inp["right"], c["macros"]["D_MIN"], c["macros"]["D_MAX"], c["w"], c["h"]


def test_main_permeability_on_tsukuba_with_host_compare(orc, main_cases, golden, tmp_path):
    left, right = golden["tsukuba0"], golden["tsukuba1"]
    h, w = left.shape[:2]
    r, files = run_ok(tmp_path, left, right, [-15, 0], ["--permeability", "--host-compare"])
    e, changed = expected(orc, left, right, -15, 0, 32.0)
    assert changed > 0                                                      # the option does something on this pair
    check_outputs(orc, files, e, w, h, "tsukuba --permeability", mean_empty=True)
    same_bits(files["png"]["disparity_mapl_perm"], orc.write_mat_u8(e["dmapl"]), "disparity_mapl_perm.png")
    check_ok_lines(r, {"Permeability ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13


@pytest.mark.parametrize("flags,sigma", [(["--permeability"], 32.0), (["--permeability", "8.5"], 8.5)], ids=["default", "8.5"])
def test_main_permeability_on_a_recorded_pair(orc, main_cases, small, tmp_path, flags, sigma):
    left, right, d_lo, d_hi, w, h = small
    r, files = run_ok(tmp_path, left, right, [d_lo, d_hi], flags + ["--host-compare"])
    e, changed = expected(orc, left, right, d_lo, d_hi, sigma)
    check_outputs(orc, files, e, w, h, " ".join(flags), mean_empty=True)
    same_bits(files["png"]["disparity_mapl_perm"], orc.write_mat_u8(e["dmapl"]), "disparity_mapl_perm.png")
    check_ok_lines(r, {"Permeability ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13


def test_main_permeability_without_host_compare_and_with_the_later_stages(orc, main_cases, small, tmp_path):
    left, right, d_lo, d_hi, w, h = small
    r, files = run_ok(tmp_path, left, right, [d_lo, d_hi], ["--permeability", "16", "--speckle", "30,1", "--wmf", "occluded"])
    e, _ = expected(orc, left, right, d_lo, d_hi, 16.0, speckle=(30, 1.0), wmf="occluded")
    check_outputs(orc, files, e, w, h, "--permeability 16 --speckle --wmf", mean_empty=True)
    check_ok_lines(r, {"Permeability ok!": 0})


@pytest.mark.parametrize("flags", [["--guidance", "rgb"], ["--cost", "census"], ["--cost", "adcensus", "--ad", "rgb"],
                                   ["--guidance", "rgb", "--cost", "census", "--uniqueness", "4", "--adjust"]],
                         ids=["rgb", "census", "adcensus_rgb", "rgb_census_uniqueness_adjust"])
def test_main_permeability_twin_agrees_under_the_other_guide_and_costs(main_cases, small, tmp_path, flags):
    """the colour guide, the costs from census codes and the stages behind the winners, each against its CPU twin"""
    left, right, d_lo, d_hi, w, h = small
    r, files = run_ok(tmp_path, left, right, [d_lo, d_hi], ["--permeability", "--host-compare"] + flags)
    check_ok_lines(r, {"Permeability ok!": 1, "Occlusion ok!": 1})
    assert "disparity_mapl_perm" in files["png"] and not files["png"]["image_mean_left"].any()


def test_main_without_permeability_writes_no_such_map(main_cases, small, tmp_path):
    left, right, d_lo, d_hi, w, h = small
    r, files = run_ok(tmp_path, left, right, [d_lo, d_hi], ["--fused"])
    assert "disparity_mapl_perm" not in files["png"] and len(files["png"]) == 12


P = ["--permeability"]
REFUSED = {   # flags -> the option stderr names
    "sgm": (P + ["--aggregation", "sgm"], "--permeability"),
    "cross": (P + ["--aggregation", "cross"], "--permeability"),
    "scanline": (P + ["--aggregation", "scanline"], "--permeability"),
    "cross_scanline": (P + ["--aggregation", "cross-scanline"], "--permeability"),
    "patchmatch": (P + ["--aggregation", "patchmatch"], "--permeability"),
    "cross_scale": (P + ["--cross-scale"], "--permeability"),
    "ngpu": (P + ["--ngpu", "1"], "--permeability"),
    "pipeline": (P + ["--fused", "--pairs", "3", "--pipeline"], "--permeability"),
    "sigma_0": (["--permeability", "0"], "--permeability"),
    "trailing_text": (["--permeability", "2x"], "--permeability"),
    "two_values": (["--permeability", "2,1"], "--permeability"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_permeability_refuses(main_cases, small, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, small[0], small[1], [small[2], small[3]], flags, name)
