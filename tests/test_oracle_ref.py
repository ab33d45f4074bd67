"""The oracle (oracle/smx_oracle.c) against the reference's OWN code, away from Tsukuba.

oracle/ref_build.py compiles the reference as host programs, one per macro set, and records what it computes for every case
of oracle/ref_cases.py in tests/golden/ref_cases/.  Here the inputs are regenerated from the table and the oracle must give
the recorded maps bit for bit and the recorded volumes hash for hash.  No GPU.  Which cases have a fixture is decided by the
reference alone (a host sanitizer on the reference's programs; oracle/REF_CASES.md lists what it threw out and why).
"""
import json
import os
import re

import numpy as np
import pytest

import ref_fixtures as rf
from oracle import ref_cases as rc

ROOT = rf.ROOT
REF = os.path.join(ROOT, "oracle", "_ref")


def documented_exclusions():
    text = open(os.path.join(ROOT, "oracle", "REF_CASES.md")).read()
    block = text.split("<!-- excluded:begin -->")[1].split("<!-- excluded:end -->")[0]
    return set(re.findall(r"^\| `(\w+)` \|", block, flags=re.M))


def _locate(name):
    def locate(key):
        p = os.path.join(REF, "cases", name + ".npz")
        if not os.path.exists(p):
            return None
        z = np.load(p)
        return z[key] if key in z.files else None
    return locate


def run_oracle(orc, c, inp):
    """What the oracle computes for a case, by fixture key."""
    m = c["macros"]
    p = rf.set_params(rf.byref_default(orc.Params, orc.lib().orc_default_params), m)
    if c["mode"] == "pair":
        Il, Ir = inp["left"], inp["right"]
        if c.get("channels", 1) >= 3:
            Il, Ir = orc.gray(Il, params=p), orc.gray(Ir, params=p)
        r = orc.stereo_pair(Il, Ir, rc.size_d(m), dminl=m["D_MIN"], dminr=-m["D_MAX"], want_cost=True, want_agg=True, params=p)
        r["grayl"], r["grayr"] = Il, Ir
        return r
    if c["mode"] == "gf":
        best, dmap = inp["best"].copy(), inp["dmap"].copy()
        _, _, mean, agg = orc.guided_filter(inp["I"], inp["cost"], c["dmin"], best=best, dmap=dmap, want_agg=True, params=p)
        return {"best": best, "dmap": dmap, "mean": mean, "agg": agg}
    if c["mode"] == "occ":
        r, d = {}, inp["dl"]
        if "dr" in inp:
            d = r["occlusion"] = orc.detect_occlusion(d, inp["dr"], c["d_occlusion"], params=p)
        r["filled"] = orc.fill_occlusion(d, c["vmin"])
        return r
    if c["mode"] == "wm":
        return {"u8": orc.write_mat_u8(inp["mat"].reshape(c["h"], c["w"]))}
    return {"gray": orc.gray(inp["rgb"].reshape(c["h"], c["w"], c["channels"]), params=p)}


@pytest.mark.parametrize("name", rf.NAMES)
def test_oracle_computes_what_the_reference_computes(orc, name):
    c, fx = rf.load(name)
    got = run_oracle(orc, c, rf.inputs(c))
    seen = rf.compare(name, fx, got, "oracle", _locate(name))
    rf.expect_all(fx, seen)


def test_the_fixtures_are_the_table_minus_the_documented_exclusions():
    excluded = documented_exclusions()
    table = {c["name"] for c in rc.CASES}
    assert excluded <= table, sorted(excluded - table)
    assert set(rf.NAMES) == table - excluded
    assert len(rf.NAMES) >= 50
    limit = os.path.getsize(os.path.join(ROOT, "tests", "golden", "tsukuba_golden.npz"))
    for n in rf.NAMES:
        assert os.path.getsize(os.path.join(rf.DIR, n + ".npz")) <= limit, n
    # an axis value whose every case was thrown out must be named as not pinnable
    text = open(os.path.join(ROOT, "oracle", "REF_CASES.md")).read()
    kept_axes = {a for c in rc.CASES if c["name"] not in excluded for a in c["axes"]}
    for a in {a for c in rc.CASES for a in c["axes"]} - kept_axes:
        assert f"not pinnable: `{a}`" in text, a


def test_tsukuba_reproduces_the_recorded_manifest():
    """the sha256 of the raw dumps of the first, uncommitted build of the reference."""
    text = open(os.path.join(ROOT, "SURVEY.md")).read()
    manifest = dict((n, h) for h, n in re.findall(r"^([0-9a-f]{64})  (\w+\.(?:f32|u8))$", text, flags=re.M))
    manifest.update((n, h) for n, h in re.findall(r"`(agg[lr]\.f32)` sha256 `([0-9a-f]{64})`", text))
    key_of = {"I_l.u8": "grayl", "I_r.u8": "grayr", "mean1.u8": "meanl", "mean2.u8": "meanr", "costl.f32": "costl",
              "costr.f32": "costr", "best_costl.f32": "bestl", "best_costr.f32": "bestr", "dmapl.f32": "dmapl",
              "dmapr.f32": "dmapr", "occlusion.f32": "occlusion", "occlusion_filled.f32": "filled", "aggl.f32": "aggl",
              "aggr.f32": "aggr"}
    assert set(manifest) == set(key_of), sorted(manifest)
    _, fx = rf.load("tsukuba")
    for fname, key in key_of.items():
        if key in fx:
            assert not (fx[key].dtype == np.float32 and np.isnan(fx[key]).any())
            got = rc.sha256_canonical(fx[key])
        else:
            got = str(fx["sha_" + key])
        assert got == manifest[fname], fname


def test_recording_again_reproduces_the_committed_fixtures():
    """With the reference present: oracle/_ref is (re)built by the committed recipe -- a no-op when its stamp is current --
    and what it records equals the committed fixtures array for array, byte for byte; what the sanitizer throws out is what
    oracle/REF_CASES.md lists.  Skips only where there is no reference to build."""
    from oracle import ref_build
    if ref_build.reference_dir() is None:
        pytest.skip("no reference directory ($SMX_REFERENCE_DIR): nothing to record from")
    assert ref_build.main() == 0
    done = json.load(open(os.path.join(REF, "STAMP")))
    assert set(done["excluded"]) == documented_exclusions()
    assert set(done["kept"]) == set(rf.NAMES)
    for v in rc.VARIANTS:
        assert os.path.exists(os.path.join(REF, "ref_" + v)) and os.path.exists(os.path.join(REF, "ref_" + v + "_san")), v
    for n in rf.NAMES:
        new, old = np.load(os.path.join(REF, "fixtures", n + ".npz")), np.load(os.path.join(rf.DIR, n + ".npz"))
        assert set(new.files) == set(old.files), n
        for k in old.files:
            a, b = new[k], old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (n, k)
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(REF) for f in fs)
    assert size < 100 << 20, size
