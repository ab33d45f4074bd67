"""The drop-in main with cross-scale aggregation (`smx_main L R DMIN DMAX OUTDIR --cross-scale [S[,LAMBDA]]`) on a 129 x 70 pair:
every file it writes against references alone -- the oracle's aggregated volumes of every level of the numpy pyramid,
tests/cscale_ref.py's combination and winners, tests/main_harness.py's chain behind them.  With --host-compare the run also
executes the twins (pyrDownOnCPU, the cost and guided-filter twins at every level, crossScaleOnCPU; the first and the last held to
cscale_ref on the CPU by tests/test_host_cscale_cpu.py) and must print "Cross-scale ok!".  Without the flag the files are those
of the plain pair, byte for byte.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_cscale
"""
import numpy as np
import pytest

import cgf_ref
import cscale_ref as ref
import main_harness
import subpix_ref
from main_harness import assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

W, H, D_LO, D_HI = 129, 70, -11, 0
D = D_HI - D_LO + 1
F32 = np.float32
PRESET = np.uint32(0x7F7F7F7F).view(F32)


@pytest.fixture(scope="module")
def scene(orc):
    left, right = cgf_ref.colour_pair(W, H, D, 2014)
    return left, right, orc.gray(left), orc.gray(right)


def plain(orc, gl, gr):
    w = orc.stereo_pair(gl, gr, D, dminl=D_LO, dminr=-D_HI, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy()}
    e.update({k: w[k] for k in ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr")})
    return e


def cross_scale(orc, gl, gr, scales, lam):
    """the maps up to dmapl / dmapr of a cross-scale pair: the mean images are empty"""
    e = plain(orc, gl, gr)
    e["meanl"], e["meanr"] = np.zeros_like(e["meanl"]), np.zeros_like(e["meanr"])
    pl, pr = ref.pyramid(gl, scales), ref.pyramid(gr, scales)
    levels = ([], [])
    for s in range(scales):
        _, _, dl, sl = ref.level(W, H, D_LO, D, s)
        _, _, dr, sr = ref.level(W, H, -D_HI, D, s)
        v = orc.stereo_pair(pl[s], pr[s], max(sl, sr), dminl=dl, dminr=dr, want_agg=True)
        levels[0].append(v["aggl"][:sl])
        levels[1].append(v["aggr"][:sr])
    for v, (side, dmin) in enumerate((("l", D_LO), ("r", -D_HI))):
        z, c0 = ref.winners(ref.combine(levels[v], dmin, D, lam))
        e["dmap" + side] = subpix_ref.dmap_of(z, c0, dmin)
        e["best" + side] = np.where((z >= 0) & (PRESET >= c0), c0, PRESET).astype(F32)
    return e


@pytest.mark.parametrize("flags,scales,lam", [(["--cross-scale"], 4, 1.0), (["--cross-scale", "2,0.3"], 2, 0.3)],
                         ids=["defaults", "2,0.3"])
def test_main_cross_scale(orc, main_cases, scene, tmp_path, flags, scales, lam):
    """--cross-scale alone implies the device-resident flow; the twin agrees"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], flags + ["--host-compare"])
    e = cross_scale(orc, gl, gr, scales, lam)
    assert np.any(e["dmapl"] != plain(orc, gl, gr)["dmapl"])                 # the option does something on this pair
    check_outputs(orc, files, main_harness.finish_chain(orc, e, D_LO, D), W, H, " ".join(flags), mean_empty=True)
    same_bits(files["png"]["disparity_mapl_cscale"], orc.write_mat_u8(e["dmapl"]), "disparity_mapl_cscale.png")
    check_ok_lines(r, {"Cross-scale ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13


def test_main_cross_scale_without_host_compare_and_with_the_later_stages(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--cross-scale", "3", "--speckle", "30,1", "--wmf", "occluded"])
    e = main_harness.finish_chain(orc, cross_scale(orc, gl, gr, 3, 1.0), D_LO, D, speckle=(30, 1.0), wmf="occluded")
    check_outputs(orc, files, e, W, H, "--cross-scale 3 --speckle --wmf", mean_empty=True)
    check_ok_lines(r, {"Cross-scale ok!": 0})


@pytest.mark.parametrize("flags", [["--guidance", "rgb"], ["--cost", "census"], ["--cost", "adcensus", "--ad", "rgb"],
                                   ["--guidance", "rgb", "--cost", "census", "--uniqueness", "4", "--adjust"]],
                         ids=["rgb", "census", "adcensus_rgb", "rgb_census_uniqueness_adjust"])
def test_main_cross_scale_twin_agrees_under_the_other_guide_and_costs(main_cases, scene, tmp_path, flags):
    """the colour pyramid, the costs from census codes and the stages behind the winners, each against its CPU twin"""
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--cross-scale", "3,0.3", "--host-compare"] + flags)
    check_ok_lines(r, {"Cross-scale ok!": 1, "Occlusion ok!": 1})
    assert "disparity_mapl_cscale" in files["png"] and not files["png"]["image_mean_left"].any()


def test_main_without_cross_scale_writes_what_it_wrote(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], [])
    check_outputs(orc, files, main_harness.finish_chain(orc, plain(orc, gl, gr), D_LO, D), W, H, "no --cross-scale")
    assert "disparity_mapl_cscale" not in files["png"] and len(files["png"]) == 12


def test_main_one_scale_writes_the_plain_maps(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], ["--cross-scale", "1"])
    e = plain(orc, gl, gr)
    e["meanl"], e["meanr"] = np.zeros_like(e["meanl"]), np.zeros_like(e["meanr"])
    check_outputs(orc, files, main_harness.finish_chain(orc, e, D_LO, D), W, H, "--cross-scale 1", mean_empty=True)


C = ["--cross-scale"]
REFUSED = {   # flags -> the option stderr names
    "sgm": (C + ["--aggregation", "sgm"], "--cross-scale"),
    "cross": (C + ["--aggregation", "cross"], "--cross-scale"),
    "scanline": (C + ["--aggregation", "scanline"], "--cross-scale"),
    "cross_scanline": (C + ["--aggregation", "cross-scanline"], "--cross-scale"),
    "ngpu": (C + ["--ngpu", "1"], "--cross-scale"),
    "ngpu_2": (C + ["--ngpu", "2"], "--cross-scale"),
    "pipeline": (C + ["--fused", "--pairs", "3", "--pipeline"], "--cross-scale"),
    "scales_0": (["--cross-scale", "0"], "--cross-scale"),
    "scales_6": (["--cross-scale", "6"], "--cross-scale"),
    "three_values": (["--cross-scale", "2,1,1"], "--cross-scale"),
    "trailing_text": (["--cross-scale", "2x"], "--cross-scale"),
    "lambda_inf": (["--cross-scale", "2,inf"], "--cross-scale"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_cross_scale_refuses(main_cases, scene, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], flags, name)
