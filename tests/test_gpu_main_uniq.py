"""The drop-in main with the uniqueness filter (`smx_main L R DMIN DMAX OUTDIR --uniqueness PCT ...`): every file it writes
against a chain of references alone -- the oracle's pair (or tests/census_ref.py + tests/sgm_ref.py), tests/uniq_ref.py,
tests/speckle_ref.py, the oracle's fill, tests/subpix_ref.py / tests/wmf_ref.py.  With --host-compare the run also executes
uniqueness_onCPU (host/cpu_twins.cpp: sec by brute force from the aggregated volume; held to uniq_ref on the CPU by
tests/test_uniq_cpu.py) and prints its line.

Run on the GPU box:  python -m pytest tests -m gpu -q -k main_uniq
"""
import os

import numpy as np
import pytest

import census_ref
import sgm_ref
import speckle_ref
import subpix_ref
import uniq_ref
import wmf_ref
from test_gpu_main_sgm import SCENES, check_ok_lines, main_cases, rgb_pair, run  # noqa: F401  (main_cases: a fixture)

pytestmark = pytest.mark.gpu

PCT = 20
SGM_PCT = 50        # (the margins of SGM's sums are wide: at 20 % the filter changes 19 pixels of this scene, at 50 % 353)


def ratio_of(pct):
    return np.float32(pct) / (np.float32(100) - np.float32(pct))


SPK = (30, 1.0)


def tail(orc, e, agg_l, d_lo, D, gl, speckle=None, subpixel=None, nbr=None, z=None, c0=None, wmf=None, pct=PCT):
    """The stages behind the LR check, in numpy: uniqueness -> speckle -> fill -> sub-pixel / weighted median."""
    zz, cc, sec = uniq_ref.second_best(agg_l)[:3]
    e["unique"], _ = uniq_ref.apply(e["occlusion"], zz >= 0, cc, sec, ratio_of(pct), d_lo, d_lo - 100)
    kept = e["unique"]
    if speckle:
        kept = e["despeckled"] = speckle_ref.speckle_filter(kept, d_lo, d_lo - 100, *speckle)
    e["filled"] = e["final"] = orc.fill_occlusion(kept, d_lo)
    if subpixel:
        _, e["sub_filled"] = subpix_ref.maps(subpix_ref.MODES[subpixel], z, c0, nbr[0], nbr[1], e["dmapl"], kept, e["filled"], d_lo)
        e["final"] = e["sub_filled"]
    if wmf:
        e["refined"] = e["final"] = wmf_ref.weighted_median(gl, e["filled"], d_lo, D, kept if wmf == "occluded" else None)
    return e


def guided_chain(orc, gl, gr, d_lo, d_hi, **kw):
    D = d_hi - d_lo + 1
    w = orc.stereo_pair(gl, gr, D, dminl=d_lo, dminr=-d_hi, want_cost=True, want_agg=True)
    e = {"grayl": gl, "grayr": gr, "cost0l": w["costl"][0].copy(), "cost0r": w["costr"][0].copy()}
    e.update({k: w[k] for k in ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr", "occlusion")})
    z, c0, lo, hi, _ = subpix_ref.winners(w["aggl"])
    return tail(orc, e, w["aggl"], d_lo, D, gl, nbr=(lo, hi), z=z, c0=c0, **kw)


def sgm_chain(orc, gl, gr, d_lo, d_hi, **kw):
    D = d_hi - d_lo + 1
    dmin = (d_lo, -d_hi)
    vols = [census_ref.census_cost(a, b, D, dm) for (a, b), dm in zip(((gl, gr), (gr, gl)), dmin)]
    sl, sr = (sgm_ref.outputs(v, 10, 120, 8) for v in vols)
    e = {"grayl": gl, "grayr": gr, "meanl": np.zeros_like(gl), "meanr": np.zeros_like(gr),
         "cost0l": vols[0][0].copy(), "cost0r": vols[1][0].copy(), "bestl": sl["best"], "bestr": sr["best"],
         "dmapl": (dmin[0] + sl["z"]).astype(np.float32), "dmapr": (dmin[1] + sr["z"]).astype(np.float32)}
    e["occlusion"] = orc.detect_occlusion(e["dmapl"], e["dmapr"], d_lo - 100)
    return tail(orc, e, sl["agg"], d_lo, D, gl, nbr=sl["nbr"], z=sl["z"], c0=sl["best"], **kw)


def check_files(orc, mc, files, e, gl, what):
    mc.check_twelve(orc, files, e, what)
    for key, fname in (("unique", "occlu_mapl_unique"), ("despeckled", "occlu_mapl_despeckled"), ("refined", "occlu_mapl_wmf")):
        if key in e:
            mc.same_bits(files["png"][fname], orc.write_mat_u8(e[key]), f"{what} {fname}.png")
        else:
            assert fname not in files["png"], (what, fname)
    mc.check_disparity_files(files, e["final"], gl.shape[1], gl.shape[0], what)
    assert np.any(e["unique"] != e["occlusion"]), what + ": the filter changed nothing on the reference values"


def scene_of(orc, name):
    left, right, gl, gr = rgb_pair(orc, name)
    return left, right, gl, gr, SCENES[name][4], SCENES[name][5], None


@pytest.mark.parametrize("host_compare", [False, True], ids=["plain", "host_compare"])
def test_main_uniqueness_guided(orc, main_cases, tmp_path, host_compare):
    scene = scene_of(orc, "main")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(main_cases, tmp_path, scene, ["--uniqueness", str(PCT), "--speckle", "30,1", "--wmf", "occluded"] +
                   (["--host-compare"] if host_compare else []))
    check_files(orc, main_cases, files, guided_chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, wmf="occluded"), gl, "guided")
    check_ok_lines(r, {"Uniqueness ok!": int(host_compare), "Occlusion ok!": int(host_compare)})


def test_main_uniqueness_alone_subpixel(orc, main_cases, tmp_path):
    scene = scene_of(orc, "x0")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(main_cases, tmp_path, scene, ["--uniqueness", str(PCT), "--subpixel", "parabola", "--host-compare"])
    check_files(orc, main_cases, files, guided_chain(orc, gl, gr, d_lo, d_hi, subpixel="parabola"), gl, "guided subpixel")
    check_ok_lines(r, {"Uniqueness ok!": 1, "Occlusion ok!": 1})


def test_main_uniqueness_census_sgm(orc, main_cases, tmp_path):
    scene = scene_of(orc, "main")
    left, right, gl, gr, d_lo, d_hi, _ = scene
    r, files = run(main_cases, tmp_path, scene, ["--uniqueness", str(SGM_PCT), "--aggregation", "sgm", "--speckle", "30,1",
                                                 "--subpixel", "parabola", "--host-compare"])
    e = sgm_chain(orc, gl, gr, d_lo, d_hi, speckle=SPK, subpixel="parabola", pct=SGM_PCT)
    check_files(orc, main_cases, files, e, gl, "census sgm")
    assert not files["png"]["image_mean_left"].any()
    check_ok_lines(r, {"Uniqueness ok!": 1, "Semi-global matching ok!": 1, "Occlusion ok!": 1})


def test_main_without_the_option_writes_the_twelve_files(orc, main_cases, tmp_path):
    """Absent (and with PCT 0, which is off) the file set and every byte are those of a plain run."""
    blobs = []
    scene = scene_of(orc, "x0")
    for sub, flags in (("plain", []), ("zero", ["--uniqueness", "0"])):
        d = tmp_path / sub
        d.mkdir()
        run(main_cases, d, scene, flags)
        names = sorted(os.listdir(d / "out"))
        assert len(names) == 12 and "occlu_mapl_unique.png" not in names, names
        blobs.append({n: (d / "out" / n).read_bytes() for n in names})
    assert blobs[0] == blobs[1]


REFUSED = {"ngpu": ["--uniqueness", "20", "--ngpu", "1"], "pipeline": ["--uniqueness", "20", "--fused", "--pairs", "3", "--pipeline"],
           "hundred": ["--uniqueness", "100"], "negative": ["--uniqueness", "-1"], "text": ["--uniqueness", "5x"],
           "nan": ["--uniqueness", "nan"], "no_value": ["--uniqueness"]}


@pytest.mark.parametrize("case", list(REFUSED))
def test_main_uniqueness_refuses(orc, main_cases, tmp_path, case):
    left, right = rgb_pair(orc, "x0")[:2]
    r, files = main_cases.run_main(main_cases.BIN, tmp_path, left, right, [-5, 6], REFUSED[case], timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout + r.stderr)
    assert "--uniqueness" in r.stderr, r.stderr
    assert not files["png"] and "pfm" not in files and "png16" not in files
