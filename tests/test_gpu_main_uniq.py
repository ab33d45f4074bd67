"""The drop-in main with the uniqueness filter (`smx_main L R DMIN DMAX OUTDIR --uniqueness PCT ...`): every file it writes
against a chain of references alone -- the oracle's pair (or tests/census_ref.py + tests/sgm_ref.py), tests/uniq_ref.py,
tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py / tests/wmf_ref.py.  With --host-compare the run also executes
uniqueness_onCPU (host/cpu_twins.cpp: sec by brute force from the aggregated volume; held to uniq_ref on the CPU by
tests/test_uniq_cpu.py) and prints its line.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_uniq
"""
import numpy as np
import pytest

import census_ref
import cgf_ref
import sgm_ref
import uniq_ref
from main_harness import (assert_refused, assert_same_files_as_plain, check_ok_lines, check_outputs, finish_chain,  # noqa: F401
                          main_cases)
from test_gpu_main_sgm import SCENES, rgb_pair, run

pytestmark = pytest.mark.gpu

PCT = 20
SGM_PCT = 50        # (the margins of SGM's sums are wide: at 20 % the filter changes 19 pixels of this scene, at 50 % 353)


SPK = (30, 1.0)


def guided_chain(orc, gl, gr, d_lo, d_hi, pct=PCT, **kw):
    D = d_hi - d_lo + 1
    w = orc.stereo_pair(gl, gr, D, dminl=d_lo, dminr=-d_hi, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy()}
    e.update({k: w[k] for k in ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr")})
    sl = cgf_ref.states(w["aggl"])
    return finish_chain(orc, e, d_lo, D, z=sl["z"], best=sl["best"], sec=sl["uq"][0], nbr=sl["nbr"], uniqueness=pct, **kw)


def sgm_chain(orc, gl, gr, d_lo, d_hi, pct=PCT, **kw):
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    vols = [census_ref.census_cost(a, b, D, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    sl, sr = (sgm_ref.outputs(v, 10, 120, 8) for v in vols)
    e = {"grayl": gl, "grayr": gr, "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr),
         "cost0l": vols[0][0].copy(), "cost0r": vols[1][0].copy(), "bestl": sl["best"], "bestr": sr["best"],
         "dmapl": (dmin[0] + sl["z"]).astype(np.float32), "dmapr": (dmin[1] + sr["z"]).astype(np.float32)}
    return finish_chain(orc, e, d_lo, D, z=sl["z"], best=sl["best"], sec=uniq_ref.second_best(sl["agg"])[2], nbr=sl["nbr"],
                        uniqueness=pct, **kw)


def check_files(orc, files, e, gl, what):
    check_outputs(orc, files, e, gl.shape[1], gl.shape[0], what)
    assert np.any(e["unique"] != e["occlusion"]), what + ": the filter changed nothing on the reference values"


def scene_of(orc, name):
    left, right, gl, gr = rgb_pair(orc, name)
    return left, right, gl, gr, SCENES[name][4], SCENES[name][5], None


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_uniqueness_guided(orc, main_cases, tmp_path, host_compare):
    scene = scene_of(orc, "main")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(tmp_path, scene, ["--uniqueness", str(PCT), "--speckle", "30,1", "--wmf", "occluded"] +
                   (["--host-compare"] if host_compare else []))
    check_files(orc, files, guided_chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, wmf="occluded"), gl, "guided")
    check_ok_lines(r, {"Uniqueness ok!": int(host_compare), "Occlusion ok!": int(host_compare)})


def test_main_uniqueness_alone_subpixel(orc, main_cases, tmp_path):
    scene = scene_of(orc, "x0")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(tmp_path, scene, ["--uniqueness", str(PCT), "--subpixel", "parabola", "--host-compare"])
    check_files(orc, files, guided_chain(orc, gl, gr, d_lo, d_hi, subpixel="parabola"), gl, "guided subpixel")
    check_ok_lines(r, {"Uniqueness ok!": 1, "Occlusion ok!": 1})


def test_main_uniqueness_census_sgm(orc, main_cases, tmp_path):
    scene = scene_of(orc, "main")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(tmp_path, scene, ["--uniqueness", str(SGM_PCT), "--aggregation", "sgm", "--speckle", "30,1",
                                                 "--subpixel", "parabola", "--host-compare"])
    e = sgm_chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, subpixel="parabola", pct=SGM_PCT)
    check_files(orc, files, e, gl, "census sgm")
    assert not files["png"]["image_mean_left"].any()
    check_ok_lines(r, {"Uniqueness ok!": 1, "Semi-global matching ok!": 1, "Occlusion ok!": 1})


def test_main_without_the_option_writes_the_twelve_files(orc, main_cases, tmp_path):
    """Absent (and with PCT 0, which is off) the file set and every byte are those of a plain run."""
    left, right = rgb_pair(orc, "x0")[:2]
    assert_same_files_as_plain(tmp_path, left, right, [-5, 6], ["--uniqueness", "0"])


REFUSED = {"ngpu": ["--uniqueness", "20", "--ngpu", "1"], "pipeline": ["--uniqueness", "20", "--fused", "--pairs", "3", "--pipeline"],
           "hundred": ["--uniqueness", "100"], "negative": ["--uniqueness", "-1"], "text": ["--uniqueness", "5x"],
           "nan": ["--uniqueness", "nan"], "no_value": ["--uniqueness"]}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_uniqueness_refuses(orc, main_cases, tmp_path, case):
    left, right = rgb_pair(orc, "x0")[:2]
    assert_refused(tmp_path, left, right, [-5, 6], REFUSED[case], "--uniqueness")
