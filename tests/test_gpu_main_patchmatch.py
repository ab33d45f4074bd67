"""The drop-in main with PatchMatch stereo (`smx_main L R DMIN DMAX OUTDIR --aggregation patchmatch [--pm-*]`) on a small pair:
every file it writes against references alone -- tests/patchmatch_ref.py's search, tests/main_harness.py's chain behind its
labels.  With --host-compare the run also executes the twin (patchMatchOnCPU, held to patchmatch_ref on the CPU by
tests/test_host_patchmatch_cpu.py) and must print "PatchMatch ok!".

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_patchmatch
"""
import functools

import numpy as np
import pytest

import main_harness
import patchmatch_ref as ref
import subpix_ref
from main_harness import assert_refused, check_ok_lines, check_outputs, main_cases, run_ok, same_bits  # noqa: F401
from test_patchmatch_cpu import default_cc

pytestmark = pytest.mark.gpu

W, H, D_LO, D_HI = 61, 30, -7, 0
D = D_HI - D_LO + 1
F32 = np.float32
PM = ["--aggregation", "patchmatch", "--pm-radius", "2", "--pm-iterations", "2", "--pm-seed", "9"]


@pytest.fixture(scope="module")
def scene(orc):
    """a gray texture as an RGB pair (so that the gray conversion is the identity up to the weights): the right view is the left
    one moved by 2 columns, a nearer block by 5"""
    rng = np.random.default_rng(2011)
    tex = rng.integers(0, 256, (H, W + 8, 3)).astype(np.uint8)
    left = tex[:, 4:4 + W].copy()
    right = left.copy()
    right[:, :W - 2] = left[:, 2:]
    right[10:22, 12:34] = left[10:22, 17:39]
    return left, right, orc.gray(left), orc.gray(right)


@functools.lru_cache(maxsize=None)
def _search(gl_bytes, gr_bytes):
    gl = np.frombuffer(gl_bytes, np.uint8).reshape(H, W)
    gr = np.frombuffer(gr_bytes, np.uint8).reshape(H, W)
    return ref.patchmatch(gl, gr, D, D_LO, -D_HI, ref.PMParams(radius=2, iterations=2, seed=9), default_cc())


def expected(orc, gl, gr, **later):
    """the maps of a PatchMatch pair: labels and plane costs in place of the winners, empty mean images, the chain behind them,
    and the fractional filled map as the final one"""
    pm = _search(gl.tobytes(), gr.tobytes())
    e = {"grayl": gl, "grayr": gr, "cost0l": orc.cost_volume(gl, gr, 1, D_LO)[0], "cost0r": orc.cost_volume(gr, gl, 1, -D_HI)[0],
         "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr), "bestl": pm["cost"][0], "bestr": pm["cost"][1],
         "dmapl": pm["label"][0], "dmapr": pm["label"][1]}
    e = main_harness.finish_chain(orc, e, D_LO, D, **later)
    kept = e.get("despeckled", e["occlusion"])
    e["final"] = np.where(subpix_ref.kept(kept, D_LO), pm["disp"][0], e["filled"]).astype(F32)
    return e, pm


def test_main_patchmatch_with_host_compare(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], PM + ["--host-compare"])
    e, pm = expected(orc, gl, gr)
    check_outputs(orc, files, e, W, H, " ".join(PM), mean_empty=True)
    same_bits(files["png"]["disparity_mapl_patchmatch"], orc.write_mat_u8(pm["disp"][0]), "disparity_mapl_patchmatch.png")
    check_ok_lines(r, {"PatchMatch ok!": 1, "Occlusion ok!": 1})
    assert len(files["png"]) == 13
    assert (e["final"] != e["filled"]).any() and (e["occlusion"] != e["dmapl"]).any()     # fractional, and the LR check dropped pixels


def test_main_patchmatch_without_host_compare_and_with_the_later_stages(orc, main_cases, scene, tmp_path):
    left, right, gl, gr = scene
    r, files = run_ok(tmp_path, left, right, [D_LO, D_HI], PM + ["--speckle", "12,1", "--wmf", "occluded"])
    e, pm = expected(orc, gl, gr, speckle=(12, 1.0), wmf="occluded")
    check_outputs(orc, files, e, W, H, "patchmatch --speckle --wmf", mean_empty=True)
    check_ok_lines(r, {"PatchMatch ok!": 0})
    assert len(files["png"]) == 15


REFUSED = {   # flags -> the option stderr names
    "census": (PM + ["--cost", "census"], "--aggregation patchmatch"),
    "adcensus": (PM + ["--cost", "adcensus"], "--aggregation patchmatch"),
    "rgb": (PM + ["--guidance", "rgb"], "--aggregation patchmatch"),
    "cross_scale": (PM + ["--cross-scale"], "--aggregation patchmatch"),
    "adjust": (PM + ["--adjust"], "--aggregation patchmatch"),
    "uniqueness": (PM + ["--uniqueness", "10"], "--aggregation patchmatch"),
    "subpixel": (PM + ["--subpixel", "parabola"], "--aggregation patchmatch"),
    "ngpu": (PM + ["--ngpu", "1"], "--aggregation patchmatch"),
    "pipeline": (PM + ["--fused", "--pairs", "3", "--pipeline"], "--aggregation patchmatch"),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_patchmatch_refuses(main_cases, scene, tmp_path, case):
    flags, name = REFUSED[case]
    assert_refused(tmp_path, scene[0], scene[1], [D_LO, D_HI], flags, name)
