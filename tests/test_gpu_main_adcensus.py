"""The drop-in main with the AD-Census cost (`smx_main L R DMIN DMAX OUTDIR --cost adcensus ...`): every file it writes
against a chain of references alone -- the oracle's gray conversion, tests/adcensus_ref.py, the oracle's guided filter (or
tests/sgm_ref.py), LR check and fill; the 8-bit images are oracle.write_mat_u8 of the expected map.  That chain is what
PairPipeline(cost="adcensus") is held to in tests/test_gpu_adcensus.py.  With --host-compare the run also executes
adcensus_costOnCPU (host/cpu_twins.cpp, held to adcensus_ref on the CPU by tests/test_host_adcensus_cpu.py) and the
check_errors wiring of host/stages.cpp around it.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_adcensus
"""
import numpy as np
import pytest

import adcensus_ref as ref
import sgm_ref
from main_harness import (assert_refused, check_disparity_files, check_ok_lines, check_twelve, finish_chain, main_cases,  # noqa: F401
                          run_ok, same_bits)
from test_gpu_adcensus import expected
from test_gpu_census import _rgb_pair

pytestmark = pytest.mark.gpu

W, H = 129, 70


def _volumes(left, right, gl, gr, D, rgb, **kw):
    if rgb:
        return (ref.cost(left, right, gl, gr, D, -(D - 1), colour=1, **kw), ref.cost(right, left, gr, gl, D, 0, colour=1, **kw))
    return ref.gray_cost(gl, gr, D, -(D - 1), **kw), ref.gray_cost(gr, gl, D, 0, **kw)


CASES = {
    "defaults": (["--cost", "adcensus"], False, {}),
    "rgb_lambda_5x3": (["--cost", "adcensus", "--ad", "rgb", "--adcensus-lambda", "20,8", "--census-window", "5x3"], True,
                       dict(rx=2, ry=1, lambda_census=20.0, lambda_ad=8.0)),
}


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
@pytest.mark.parametrize("case", list(CASES))
def test_main_writes_the_adcensus_maps(orc, main_cases, tmp_path, case, host_compare):
    flags, rgb, kw = CASES[case]
    left, right, gl, gr, D = _rgb_pair(orc)
    costs = _volumes(left, right, gl, gr, D, rgb, **kw)
    e = dict(expected(orc, gl, gr, D, -(D - 1), 0, 9, costs=costs, tag="main " + case))
    e.update(grayl=gl, grayr=gr, cost0l=e["costl"][0].copy(), cost0r=e["costr"][0].copy())
    r, files = run_ok(tmp_path, left, right, [-(D - 1), 0], flags + (["--host-compare"] if host_compare else []))
    check_twelve(orc, files, e, " ".join(flags))
    check_disparity_files(files, e["filled"], W, H, " ".join(flags))
    assert len(np.unique(e["dmapl"])) > 3 and (e["occlusion"] == -(D - 1) - 100).any()
    check_ok_lines(r, {line: count if host_compare else 0 for line, count in
                       {"Grayscale ok!": 2, "AD-Census cost ok!": 2, "Occlusion ok!": 1}.items()})


def test_the_two_cases_differ(orc):
    """The options reach the cost: the second case's volume is another one (the test above would pass on nothing otherwise)."""
    left, right, gl, gr, D = _rgb_pair(orc)
    a = _volumes(left, right, gl, gr, D, False)
    b = _volumes(left, right, gl, gr, D, True, **CASES["rgb_lambda_5x3"][2])
    c = _volumes(left, right, gl, gr, D, True)
    assert np.any(a[0] != b[0]) and np.any(b[0] != c[0]) and np.any(a[0] != c[0])


def test_main_adcensus_with_semi_global_matching(orc, main_cases, tmp_path):
    """--cost adcensus keeps its cost under --aggregation sgm (which implies census only where no --cost is given)."""
    left, right, gl, gr, D = _rgb_pair(orc)
    cl, cr = _volumes(left, right, gl, gr, D, False)
    sl, sr = sgm_ref.outputs(cl), sgm_ref.outputs(cr)
    e = finish_chain(orc, dict(bestl=sl["best"], bestr=sr["best"], dmapl=(-(D - 1) + sl["z"]).astype(np.float32),
                               dmapr=sr["z"].astype(np.float32)), -(D - 1), D)
    e.update(grayl=gl, grayr=gr, meanl=np.zeros_like(gl), meanr=np.zeros_like(gr), cost0l=cl[0].copy(), cost0r=cr[0].copy())
    r, files = run_ok(tmp_path, left, right, [-(D - 1), 0], ["--cost", "adcensus", "--aggregation", "sgm", "--host-compare"])
    check_twelve(orc, files, e, "adcensus sgm")
    check_disparity_files(files, e["filled"], W, H, "adcensus sgm")
    check_ok_lines(r, {"Semi-global matching ok!": 1, "AD-Census cost ok!": 2})


def test_main_adcensus_colour_with_the_colour_guide_and_the_later_stages(orc, main_cases, tmp_path):
    """--ad rgb with --guidance rgb, --uniqueness, --speckle and --subpixel: tests/cgf_ref.py on the colour AD-Census volumes
    and the references of the later stages (the chain of tests/test_gpu_adcensus.py); --pfm / --png16 hold the sub-pixel map."""
    import cgf_ref
    from test_gpu_adcensus import SPK, chain
    pct = 13.0
    left, right, gl, gr, D = _rgb_pair(orc)
    cl, cr = _volumes(left, right, gl, gr, D, True)
    ratio = np.float32(pct) / (np.float32(100.0) - np.float32(pct))           # main.cpp: pct / (100.0f - pct)
    e = chain(orc, gl, cgf_ref.aggregate(left, cl), cgf_ref.aggregate(right, cr), D, -(D - 1), ratio=ratio)
    e.update(grayl=gl, grayr=gr, meanl=np.zeros_like(gl), meanr=np.zeros_like(gr), cost0l=cl[0].copy(), cost0r=cr[0].copy())
    flags = ["--cost", "adcensus", "--ad", "rgb", "--guidance", "rgb", "--uniqueness", str(pct), "--speckle", "%d,%g" % SPK,
             "--subpixel", "parabola", "--host-compare"]
    r, files = run_ok(tmp_path, left, right, [-(D - 1), 0], flags)
    check_twelve(orc, files, e, " ".join(flags))
    for key, fname in (("unique", "occlu_mapl_unique"), ("despeckled", "occlu_mapl_despeckled")):
        same_bits(files["png"][fname], orc.write_mat_u8(e[key]), fname)
    check_disparity_files(files, e["subpix_filled"], W, H, " ".join(flags))
    assert np.any(e["unique"] != e["occlusion"]) and np.any(e["subpix_filled"] != np.trunc(e["subpix_filled"]))
    check_ok_lines(r, {"AD-Census cost ok!": 2, "Colour guided filter ok!": 1, "Uniqueness ok!": 1, "Occlusion ok!": 1})


REFUSED = {
    "ngpu": ["--cost", "adcensus", "--ngpu", "1"],
    "pipeline": ["--cost", "adcensus", "--fused", "--pairs", "3", "--pipeline"],
    "lambda_without_cost": ["--adcensus-lambda", "20,8"],
    "scale_without_cost": ["--adcensus-scale", "64"],
    "ad_without_cost": ["--ad", "rgb"],
    "lambda_with_census": ["--cost", "census", "--adcensus-lambda", "20,8"],
    "bad_lambda": ["--cost", "adcensus", "--adcensus-lambda", "0,8"],
    "one_lambda": ["--cost", "adcensus", "--adcensus-lambda", "20"],
    "bad_scale": ["--cost", "adcensus", "--adcensus-scale", "1e7"],
    "bad_ad": ["--cost", "adcensus", "--ad", "colour"],
    "even_window": ["--cost", "adcensus", "--census-window", "4x3"],
    "unknown_cost": ["--cost", "hamming"],
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_refuses(orc, main_cases, tmp_path, case):
    left, right, _, _, D = _rgb_pair(orc)
    r = assert_refused(tmp_path, left, right, [-(D - 1), 0], REFUSED[case], ("--cost", "--adcensus", "--ad ", "--census"))
    if case in ("ngpu", "pipeline", "unknown_cost"):
        assert "--cost" in r.stderr, r.stderr
