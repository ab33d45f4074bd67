"""The drop-in main with the mutual-information cost (`smx_main L R DMIN DMAX OUTDIR --cost mi ...`): every file it writes
against a chain of references alone -- the oracle's gray conversion, the loop of tests/mi_ref.py around the oracle's guided
filter (or tests/sgm_ref.py), LR check and fill; the 8-bit images are oracle.write_mat_u8 of the expected map.  With
--host-compare the run also recomputes the last table from its histogram, executes mi_costOnCPU (host/cpu_twins.cpp, held to
mi_ref on the CPU by tests/test_host_mi_cpu.py) and feeds the aggregation twins with the last table's volumes.

The right image of the pair is inverted: the reference's cost does not find its labels.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_mi
"""
import numpy as np
import pytest

import mi_ref as ref
import sgm_ref
from main_harness import assert_refused, check_disparity_files, check_ok_lines, check_twelve, main_cases, run_ok  # noqa: F401
from test_gpu_census import _rgb_pair

pytestmark = pytest.mark.gpu

W, H = 129, 70
F32 = np.float32


def _pair(orc):
    left, right, gl, _, D = _rgb_pair(orc)
    right = (255 - right).astype(np.uint8)
    return left, right, gl, orc.gray(right), D


def _solver(orc, gl, gr, D, sgm):
    dminl = -(D - 1)

    def solve(cl, cr):
        if sgm:
            sl, sr = sgm_ref.outputs(cl), sgm_ref.outputs(cr)
            r = dict(bestl=sl["best"], bestr=sr["best"], dmapl=(dminl + sl["z"]).astype(F32), dmapr=sr["z"].astype(F32),
                     meanl=np.zeros_like(gl), meanr=np.zeros_like(gr))
        else:
            bl, ml, meanl, _ = orc.guided_filter(gl, cl, dminl)
            br, mr, meanr, _ = orc.guided_filter(gr, cr, 0)
            r = dict(bestl=bl, bestr=br, dmapl=ml, dmapr=mr, meanl=meanl, meanr=meanr)
        r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], dminl - 100)
        r["filled"] = orc.fill_occlusion(r["occlusion"], float(dminl))
        return r
    return solve


_EXPECTED = {}


def expected(orc, sgm, iterations, init, seed):
    key = (sgm, iterations, init, seed)
    if key not in _EXPECTED:
        left, right, gl, gr, D = _pair(orc)
        e = dict(ref.pair_loop(gl, gr, D, -(D - 1), 0, _solver(orc, gl, gr, D, sgm), iterations, init, seed,
                               lambda: (orc.cost_volume(gl, gr, D, -(D - 1)), orc.cost_volume(gr, gl, D, 0)))[-1])
        T = e["table"]
        e.update(grayl=gl, grayr=gr, cost0l=ref.cost(T, gl, gr, 1, -(D - 1))[0], cost0r=ref.cost(T, gl, gr, 1, 0, right=True)[0])
        _EXPECTED[key] = e
    return _EXPECTED[key]


CASES = {
    "defaults": (["--cost", "mi"], False, 3, ref.INIT_RANDOM, 0),
    "one_table_reference_start": (["--cost", "mi", "--mi-iterations", "1", "--mi-init", "reference"], False, 1, ref.INIT_REFERENCE, 0),
    "two_tables_seed_5": (["--cost", "mi", "--mi-iterations", "2", "--mi-seed", "5"], False, 2, ref.INIT_RANDOM, 5),
    "sgm": (["--cost", "mi", "--aggregation", "sgm"], True, 3, ref.INIT_RANDOM, 0),
}


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
@pytest.mark.parametrize("case", list(CASES))
def test_main_writes_the_mi_maps(orc, main_cases, tmp_path, case, host_compare):
    flags, sgm, iterations, init, seed = CASES[case]
    left, right, gl, gr, D = _pair(orc)
    e = expected(orc, sgm, iterations, init, seed)
    r, files = run_ok(tmp_path, left, right, [-(D - 1), 0], flags + (["--host-compare"] if host_compare else []))
    check_twelve(orc, files, e, " ".join(flags))
    check_disparity_files(files, e["filled"], W, H, " ".join(flags))
    lines = {"Grayscale ok!": 2, "Mutual-information table ok!": 1, "Mutual-information cost ok!": 2, "Occlusion ok!": 1}
    if sgm:
        lines["Semi-global matching ok!"] = 1
    check_ok_lines(r, {line: count if host_compare else 0 for line, count in lines.items()})
    assert "error in the mutual-information" not in r.stdout


def test_the_cases_differ_and_the_reference_cost_fails_here(orc):
    """The options reach the loop (other tables, other maps), and the pair is one the feature is for."""
    left, right, gl, gr, D = _pair(orc)
    a, b, c = (expected(orc, *CASES[k][1:]) for k in ("defaults", "one_table_reference_start", "two_tables_seed_5"))
    assert np.any(a["table"] != b["table"]) and np.any(a["table"] != c["table"]) and np.any(a["dmapl"] != b["dmapl"])
    plain = orc.stereo_pair(gl, gr, D, dminl=-(D - 1), dminr=0)
    assert np.count_nonzero(plain["dmapl"] != a["dmapl"]) > W * H // 2


REFUSED = {
    "ngpu": ["--cost", "mi", "--ngpu", "1"],
    "pipeline": ["--cost", "mi", "--fused", "--pairs", "3", "--pipeline"],
    "patchmatch": ["--cost", "mi", "--aggregation", "patchmatch"],
    "iterations_without_cost": ["--mi-iterations", "2"],
    "seventeen": ["--cost", "mi", "--mi-iterations", "17"],
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_refuses(orc, main_cases, tmp_path, case):
    left, right, _, _, D = _pair(orc)
    assert_refused(tmp_path, left, right, [-(D - 1), 0], REFUSED[case], ("--cost mi", "--mi-"))
