"""The generator of the opt-in fuzz (tests/fuzz_scenes.py) on the numpy references alone: no GPU.

tests/test_gpu_optin_fuzz.py runs the committed seeds of every stage through the device entries; what it proves depends on what
those seeds hold.  This file asserts that over exactly those seeds: every draw lies inside the contract of include/smx.h (so
no case is refused or skipped), the regimes that uniform noise never reaches are reached, and no reference call is slow.  Where
one of these fails, the generator or the seed base changes -- never what the kernels are held to.
"""
import functools
import os
import time

import numpy as np
import pytest

import cross_ref
import fuzz_scenes as fs
import speckle_ref
import uniq_ref
import wmf_ref

SEEDS = range(fs.SEEDS)
TIMES = {}


@functools.lru_cache(maxsize=None)
def _case(stage, seed):
    return fs.draw(stage, seed)


@functools.lru_cache(maxsize=None)
def _reference(stage, seed):
    import oracle
    oracle.build()
    t = time.perf_counter()
    r = fs.reference(stage, _case(stage, seed), orc=oracle)
    TIMES[stage, seed] = time.perf_counter() - t
    return r


@pytest.mark.parametrize("stage", fs.STAGES)
def test_every_draw_is_inside_the_contract_and_the_same_twice(stage):
    for seed in SEEDS:
        c = fs.draw(stage, seed)
        assert fs.accepted(stage, c), (stage, seed, c["text"])
        again = _case(stage, seed)
        assert c["text"] == again["text"]
        for k, v in c.items():
            both = zip(v, again[k]) if isinstance(v, (tuple, list)) else ((v, again[k]),)
            for a, b in both:
                if isinstance(a, np.ndarray):
                    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (stage, seed, k)
    # another base gives other cases
    assert fs.draw(stage, 0, base=7)["text"] != fs.draw(stage, 0)["text"]


def test_the_gpu_file_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_optin_fuzz.py")).read()
    for word in ("pytest.skip", "importorskip", "skipif", "xfail"):
        assert word not in src, word


@pytest.mark.parametrize("stage", fs.STAGES)
def test_no_reference_call_is_slow(stage):
    for seed in SEEDS:
        _reference(stage, seed)
        assert TIMES[stage, seed] < 2.0, (stage, seed, TIMES[stage, seed], _case(stage, seed)["text"])


def test_shapes_cross_the_tile_constants():
    """every stage's seeds hold a width on an edge of its column tiles and one that is not, and more than one tile"""
    for stage in fs.STAGES:
        cols = fs.TILES[stage][0]
        ws = [_case(stage, s)["w"] for s in SEEDS]
        edges = set(fs.edge_list(cols, 1, 330))
        assert any(w in edges for w in ws) and any(w not in edges for w in ws), (stage, ws)
        assert any(w > min(cols) for w in ws), (stage, ws)


def test_cross_arms_of_every_length_and_both_thresholds_at_work():
    every, second = [], []
    for seed in SEEDS:
        c = _case("cross", seed)
        arms = _reference("cross", seed)["arms"]
        if c["l1"] == 63 and any(set(np.unique(a).tolist()) == set(range(64)) for a in arms):
            every.append(seed)
        loose = cross_ref.arms(c["guides"][0], c["l1"], c["l1"], c["tau1"], c["tau1"])
        if not np.array_equal(loose, arms[0]):
            second.append(seed)
    assert every, "no seed with l1 = 63 has arms of every length 0 .. 63"
    assert second, "in no seed do l2 / tau2 cut an arm that l1 / tau1 alone would not"


def _speckle_share(seed):
    c = _case("speckle", seed)
    valid = speckle_ref.counts(c["disp"], c["dmin"])
    out = _reference("speckle", seed)["out"]
    gone = valid & ~speckle_ref.counts(out, c["dmin"])
    return int(gone.sum()), int(valid.sum())


def test_speckle_invalidates_nothing_everything_and_something():
    shares = [_speckle_share(s) for s in SEEDS]
    assert all(v > 0 for _, v in shares)
    assert any(g == 0 for g, v in shares), shares
    assert any(g == v for g, v in shares), shares
    assert any(0 < g < v for g, v in shares), shares


def _tie_across_launches(q, launches):
    """a pixel whose smallest cost occurs in two slices of different launches"""
    with np.errstate(invalid="ignore"):
        m = np.nanmin(np.where(np.isnan(q), np.inf, q), axis=0)
        hit = q == m[None]
    per_launch = np.stack([hit[a:b].any(axis=0) for a, b in launches])
    return bool((per_launch.sum(axis=0) >= 2).any())


@pytest.mark.parametrize("stage", ["cgf", "cross", "wta"])
def test_a_tie_of_the_winner_spans_two_launches(stage):
    found = []
    for seed in SEEDS:
        c, r = _case(stage, seed), _reference(stage, seed)
        form = c["form"]
        if stage == "wta":          # (its workspace bound is not exact for the fused walkers: the calls and the explicit bound are)
            step = form["bound"] or c["D"]
            launches = [(s, min(s1, s + step)) for s0, s1 in form["ranges"] for s in range(s0, s1, step)]
            vols = (r["aggl"], r["aggr"])
        else:
            launches = fs.launches(form)
            vols = [r["q"][v] for v in fs._views(form["views"])]
        if len(launches) > 1 and any(_tie_across_launches(q, launches) for q in vols):
            found.append(seed)
    assert found, stage


def test_uniqueness_rejects_some_winners_and_keeps_some():
    between = 0
    for seed in SEEDS:
        c, r = _case("wta", seed), _reference("wta", seed)
        st = r["states"][0]
        has, c0 = uniq_ref.key_fields(st["keys"])
        rej = uniq_ref.rejects(has, c0, st["uq"][0], c["ratio"])
        between += 0 < int(rej.sum()) < int(has.sum())
    assert 2 * between >= fs.SEEDS, between


def test_weighted_median_second_level_and_empty_tiles():
    assert any(_case("wmf", s)["D"] > 64 for s in SEEDS)
    empty = []
    for seed in SEEDS:
        c = _case("wmf", seed)
        if c["mode"] != "occluded":
            continue
        sel = wmf_ref.selected(c["select"], c["dmin"], c["disp"].shape)
        tiles = [sel[y:y + 8, x:x + 64].any() for y in range(0, c["h"], 8) for x in range(0, c["w"], 64)]
        if not all(tiles) and any(tiles):
            empty.append(seed)
    assert empty, "no 'occluded' seed has a 64 x 8 tile without a selected pixel beside one with"
    # the refinement does something in most seeds
    changed = sum(not np.array_equal(_reference("wmf", s)["out"].view(np.uint32), _case("wmf", s)["disp"].view(np.uint32))
                  for s in SEEDS)
    assert 2 * changed >= fs.SEEDS, changed


def test_call_forms_cover_every_kind():
    forms = [_case(st, s)["form"] for st in ("cgf", "cross") for s in SEEDS]
    assert {f["views"] for f in forms} == {"both", "left", "right"}
    assert {len(f["ranges"]) for f in forms} == {1, 2, 3}
    for k in ("agg", "nbr", "uq"):
        assert {f["outs"][k] for f in forms} == {False, True}
    assert any(f["bound"] == 0 for f in forms) and any(0 < f["bound"] < f["c"] for f in forms)
    assert any(f["c"] == 1 for f in forms)
    assert {_case("wta", s)["path"] for s in SEEDS} == {5, 3, 1}
    assert {_case("sgm", s)["D"] for s in SEEDS} & set(fs.SGM_D)
    for stage in ("census", "adcensus"):
        rs = [(_case(stage, s)["s0"], _case(stage, s)["s1"]) for s in SEEDS]
        assert any(a == b for a, b in rs) and any((b - a) % 16 for a, b in rs), (stage, rs)


def test_compositions_cover_every_cost_and_aggregation():
    import oracle
    oracle.build()
    cases = [fs.composition(s) for s in SEEDS]
    sets = {(c["opt"]["cost"], c["opt"]["agg"], c["opt"]["subpixel"], c["opt"]["uniqueness"], c["opt"]["speckle"], c["opt"]["wmf"],
             c["opt"]["sif"]) for c in cases}
    assert len(sets) >= 12
    assert {c["opt"]["cost"] for c in cases} == set(fs.COSTS) and {c["opt"]["agg"] for c in cases} == set(fs.AGGS)
    assert all(fs.composition_ok(c["opt"]["cost"], c["opt"]["agg"]) for c in cases)
    assert len({(c["w"], c["h"], c["D"]) for c in cases}) == 1                    # one context serves them all
    for k, values in (("subpixel", 3), ("wmf", 3), ("volumes", 2)):
        assert len({c["opt"][k] for c in cases}) == values, k
    assert {bool(c["opt"]["speckle"]) for c in cases} == {False, True} == {bool(c["opt"]["uniqueness"]) for c in cases}
    rejected = despeckled = 0
    for c in cases:
        t = time.perf_counter()
        e = fs.composition_reference(c, oracle)
        assert time.perf_counter() - t < 2.0, c["text"]
        rejected += "unique" in e and bool((e["unique"] != e["occlusion"]).any())
        despeckled += "despeckled" in e and bool((e["despeckled"] != e.get("unique", e["occlusion"])).any())
        assert cross_ref.params_ok(**c["opt"]["cross"]) and fs.census_ok(**c["opt"]["census"])
    assert rejected and despeckled, (rejected, despeckled)
