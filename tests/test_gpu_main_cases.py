"""The drop-in main (`smx_main LEFT RIGHT DMIN DMAX OUTDIR [options]`) away from Tsukuba: RGB(A) pairs of other shapes and
label ranges, written as PNGs, through the binary, and every file it writes against what the reference's own code recorded
for that pair (tests/golden/ref_cases/cli_*.npz, oracle/ref_cases.py).

Where an expected value is not a recorded array it is the oracle's, and the oracle's array is first held to the recorded
sha256 (gray images, cost volumes, aggregated volumes, the best-cost maps of the KITTI shape).  The 8-bit images are
oracle.write_mat_u8 of the expected map; tests/test_host_mirror.py ties that function to the reference's write_mat.  The
weighted median and the sub-pixel maps come from tests/wmf_ref.py and tests/subpix_ref.py.  Nothing expected comes from
the library or the binary.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_cases
"""
import os
import subprocess

import numpy as np
import pytest

import ref_fixtures as rf
import subpix_ref
import wmf_ref
from main_harness import PNGS, binary, check_disparity_files, check_twelve, run_main, run_ok, same_bits, write_png  # noqa: F401  (a fixture)
from oracle import ref_cases as rc

CLI = [n for n in rf.names("pair") if n.startswith("cli_")]
ONE_LABEL = "cli_one_64x9"
CROSSES_ZERO = "cli_x0_210x150"
KITTI = "cli_kitti_1242x375"
ALL_MODES = ["cli_d70_129x70", "cli_nz_210x150", CROSSES_ZERO]       # the cases that run every flag set
FLOAT_MAPS = ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")

BASE_FLAGS = [[], ["--fused"]]
MODE_FLAGS = [["--host-compare"], ["--fused", "--host-compare"], ["--ngpu", "1"], ["--fused", "--pairs", "3"],
              ["--fused", "--pairs", "3", "--pipeline"]]


def test_the_case_table_holds_what_this_module_needs():
    assert {"cli_d70_129x70", "cli_r9_210x150", "cli_19x40", "cli_2x1", KITTI, "cli_nz_210x150", CROSSES_ZERO,
            ONE_LABEL} <= set(CLI)
    ranges = {n: (rc.BY_NAME[n]["macros"]["D_MIN"], rc.BY_NAME[n]["macros"]["D_MAX"]) for n in CLI}
    assert ranges["cli_nz_210x150"] == (-40, -6) and ranges[CROSSES_ZERO] == (-5, 6) and ranges[ONE_LABEL] == (-4, -4)
    assert ranges["cli_d70_129x70"] == (-69, 0) and ranges["cli_r9_210x150"] == (-23, 0) and ranges[KITTI] == (-31, 0)
    assert rc.BY_NAME["cli_r9_210x150"]["channels"] == 4
    for n in CLI:                           # only the range differs from what smx_main is built with
        assert {k: v for k, v in rc.BY_NAME[n]["macros"].items() if k not in ("D_MIN", "D_MAX")} == \
               {k: v for k, v in rc.DEFAULTS.items() if k not in ("D_MIN", "D_MAX")}, n


# ---- what is expected of a case --------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(orc, name):
    """{key: array} of a recorded case: the recorded maps; the gray images, the first cost slices, the aggregated volumes
    and maps recorded as hashes from the oracle, after the oracle's whole result has been held to the recording."""
    if name not in _EXPECTED:
        c, fx = rf.load(name)
        m = c["macros"]
        inp = rf.inputs(c)
        gl, gr = orc.gray(inp["left"]), orc.gray(inp["right"])
        r = orc.stereo_pair(gl, gr, rc.size_d(m), dminl=m["D_MIN"], dminr=-m["D_MAX"], want_cost=True, want_agg=True)
        r["grayl"], r["grayr"] = gl, gr
        rf.expect_all(fx, rf.compare(name, fx, r, "oracle"))          # sha_grayl/r, sha_costl/r, sha_aggl/r and every map
        e = {k: fx[k] if k in fx else r[k] for k in ("meanl", "meanr") + FLOAT_MAPS}
        e.update(grayl=gl, grayr=gr, cost0l=r["costl"][0].copy(), cost0r=r["costr"][0].copy(), aggl=r["aggl"],
                 left=inp["left"], right=inp["right"], case=c)
        _EXPECTED[name] = e
    return _EXPECTED[name]


def levels_wrap(m):
    """True where the reference's normaliser (main.cu:13-35) gives some element of the map a negative level: an element
    below its `min`, which skips every element that raised the running maximum."""
    v = np.asarray(m, np.float32).ravel()
    before = np.concatenate(([np.float32(-150000000.0)], np.maximum.accumulate(v)[:-1]))
    rest = v[~(v > np.maximum(before, np.float32(-150000000.0)))]
    lo = min(np.float32(150000000.0), rest.min()) if rest.size else np.float32(150000000.0)
    return bool(v.max() > lo and (v < lo).any())


# ---- guards: the recordings are not trivially easy ------------------------------------------------------------------------
def test_recorded_cases_have_occlusions_and_more_than_one_label():
    for name in CLI:
        c, fx = rf.load(name)
        occluded = int((fx["occlusion"] == c["macros"]["D_MIN"] - 100).sum())
        assert 0 < occluded < c["w"] * c["h"], (name, occluded)
        for k in ("dmapl", "dmapr"):
            labels = np.unique(fx[k])
            assert len(labels) >= 2 or name == ONE_LABEL, (name, k, labels)
        if name == ONE_LABEL:
            assert np.all(fx["dmapl"] == -4.0) and np.all(fx["dmapr"] == 4.0)


def test_recorded_maps_reach_the_wrapped_levels_of_the_normaliser(orc):
    wm = [n for n in rf.names("wm") if levels_wrap(rf.inputs(rf.load(n)[0])["mat"])]
    assert wm, "no kept wm case has a negative level"
    for n in wm:                              # a wrapped level is a high byte where the smallest value sits
        c, fx = rf.load(n)
        mat = rf.inputs(c)["mat"]
        assert fx["u8"].ravel()[np.argmin(mat)] > 128, n
    found = []
    for name in sorted(set(CLI) - {KITTI}):
        e = expected(orc, name)
        found += [(name, k) for k in FLOAT_MAPS + ("cost0l", "cost0r") if levels_wrap(e[k])]
    assert found, "no map of a cli case has a negative level"


# ---- running the binary -------------------------------------------------------------------------------------------------
def run_case(orc, binary, tmp_path, name, flags):
    e = expected(orc, name)
    m = e["case"]["macros"]
    r, files = run_ok(tmp_path, e["left"], e["right"], [m["D_MIN"], m["D_MAX"]], flags, timeout=300)
    assert f"Resolution : {e['case']['w']}x{e['case']['h']}" in r.stdout
    return e, r, files


def _id(flags):
    return "_".join(f.lstrip("-") for f in flags) or "stages"


# ---- every case: the per-stage host path (where smx_config() sizes the volume) and the fused one -------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flags", BASE_FLAGS, ids=_id)
@pytest.mark.parametrize("name", CLI)
def test_main_writes_what_the_reference_computes(orc, binary, tmp_path, name, flags):
    e, r, files = run_case(orc, binary, tmp_path, name, flags)
    what = f"{name} {_id(flags)}"
    check_twelve(orc, files, e, what)
    check_disparity_files(files, e["filled"], e["case"]["w"], e["case"]["h"], what)
    if name == ONE_LABEL:                   # constant maps: the zeros host/helpers.cuh defines
        for fname in ("disparity_mapl", "disparity_mapr", "occlu_mapl_filled"):
            assert e[PNGS[fname]].min() == e[PNGS[fname]].max()
            assert not files["png"][fname].any(), fname
        assert files["png"]["occlu_mapl"].any()
    if name == CROSSES_ZERO:                # positive labels: negative "disparities" in the PFM, clipped in the 16-bit PNG
        d = files["pfm"][1]
        assert (d < 0).any() and (d > 0).any()
        assert not files["png16"][d < 0].any() and files["png16"][d > 0].all()


# ---- the other modes at three ranges -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flags", MODE_FLAGS, ids=_id)
@pytest.mark.parametrize("name", ALL_MODES)
def test_main_modes(orc, binary, tmp_path, name, flags):
    e, r, files = run_case(orc, binary, tmp_path, name, flags)
    what = f"{name} {_id(flags)}"
    if "--host-compare" in flags:           # every self-check the path runs prints its line
        oks = {"Grayscale ok!": 2, "Occlusion ok!": 1} if "--fused" in flags else \
              {"Grayscale ok!": 2, "Cost volume ok!": 2, "Guided filter ok!": 2}
        for line, count in oks.items():
            assert r.stdout.count(line) == count, (what, line, r.stdout[-2000:])
    if "--pairs" in flags:
        assert "pairs 2 on one context" in r.stdout, r.stdout
        assert ("(pipelined entry)" in r.stdout) == ("--pipeline" in flags)
    check_twelve(orc, files, e, what)
    check_disparity_files(files, e["filled"], e["case"]["w"], e["case"]["h"], what)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["occluded", "all"])
@pytest.mark.parametrize("name", ALL_MODES)
def test_main_weighted_median(orc, binary, tmp_path, name, mode):
    e, r, files = run_case(orc, binary, tmp_path, name, ["--wmf", mode])
    m = e["case"]["macros"]
    want = wmf_ref.weighted_median(e["grayl"], e["filled"], m["D_MIN"], rc.size_d(m), e["occlusion"] if mode == "occluded" else None)
    assert np.any(want != e["filled"]), "the refinement changes nothing: the case checks nothing"
    what = f"{name} wmf {mode}"
    same_bits(files["png"]["occlu_mapl_wmf"], orc.write_mat_u8(want), what + " occlu_mapl_wmf.png")
    check_twelve(orc, files, e, what)
    check_disparity_files(files, want, e["case"]["w"], e["case"]["h"], what)


@pytest.mark.gpu
@pytest.mark.parametrize("fit", ["parabola", "equiangular"])
@pytest.mark.parametrize("name", ALL_MODES)
def test_main_subpixel(orc, binary, tmp_path, name, fit):
    e, r, files = run_case(orc, binary, tmp_path, name, ["--subpixel", fit])
    m = e["case"]["macros"]
    z, c0, lo, hi, _ = subpix_ref.winners(e["aggl"])
    same_bits(subpix_ref.dmap_of(z, c0, m["D_MIN"]), e["dmapl"], "the winners of the recorded volume")
    _, want = subpix_ref.maps(subpix_ref.MODES[fit], z, c0, lo, hi, e["dmapl"], e["occlusion"], e["filled"], m["D_MIN"])
    assert np.any(want != np.trunc(want)), "no fractional disparity: the case checks nothing"
    what = f"{name} subpixel {fit}"
    check_twelve(orc, files, e, what)
    check_disparity_files(files, want, e["case"]["w"], e["case"]["h"], what)


# ---- refusals and the forms of the command line --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["gray", "sizes", "missing"])
def test_main_refuses_what_is_not_an_rgb_pair(binary, tmp_path, what):
    rng = np.random.default_rng(7)
    left = rng.integers(0, 256, size=(12, 20, 3), dtype=np.uint8)
    right = rng.integers(0, 256, size=(12, 20, 3), dtype=np.uint8)
    if what == "gray":
        left = left[:, :, 0]
    if what == "sizes":
        right = right[:, :19]
    r, files = run_main(binary, tmp_path, left, right, [-3, 0], timeout=120) if what != "missing" else (None, None)
    if what == "missing":
        (tmp_path / "out").mkdir()
        L = write_png(tmp_path / "left.png", left)
        r = subprocess.run([binary, L, str(tmp_path / "no_such.png"), "-3", "0", str(tmp_path / "out")], cwd=tmp_path,
                           capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot load an RGB pair" in r.stderr, (r.returncode, r.stdout + r.stderr)
    assert not os.listdir(tmp_path / "out")


@pytest.mark.gpu
def test_main_refuses_4097_labels(binary, tmp_path):
    r = subprocess.run([binary, "a.png", "b.png", "-4096", "0", str(tmp_path)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "bad disparity range" in r.stderr, (r.returncode, r.stdout + r.stderr)


@pytest.mark.gpu
def test_three_positional_arguments_take_the_paths_and_the_default_range(orc, binary, golden, tsukuba_gray, tsukuba_oracle,
                                                                         tmp_path):
    """main.cpp: `smx_main L.png R.png [dmin dmax [outdir]]` -- a range needs both ends, so a lone third argument changes
    nothing: the pair is read from the two paths, the labels are the built-in -15..0 and the images go to ./data."""
    data = tmp_path / "data"
    r, files = run_main(binary, tmp_path, golden["tsukuba0"], golden["tsukuba1"], [-3], outdir=data)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Resolution : 384x288" in r.stdout
    e = {k: tsukuba_oracle[k] for k in ("meanl", "meanr") + FLOAT_MAPS}
    e.update(grayl=tsukuba_gray[0], grayr=tsukuba_gray[1], cost0l=tsukuba_oracle["costl"][0], cost0r=tsukuba_oracle["costr"][0])
    assert set(np.unique(e["dmapl"])) - set(np.arange(-3.0, 1.0)), "the default range must differ from -3..0 in its result"
    check_twelve(orc, files, e, "tsukuba by path")
    check_disparity_files(files, e["filled"], 384, 288, "tsukuba by path")
