"""The generator of the opt-in fuzz (tests/fuzz_scenes.py) on the numpy references alone: no GPU.

tests/test_gpu_optin_fuzz.py runs the committed seeds of every stage through the device entries; what it proves depends on what
those seeds hold.  This file asserts that over exactly those seeds: every draw lies inside the contract of include/smx.h (so
no case is refused or skipped), the regimes that uniform noise never reaches are reached, and no reference call is slow.  Where
one of these fails, the generator or the seed base changes -- never what the kernels are held to.  The last section does the
same for the table family of compositions: its draws against tests/ctx_plan_ref.py, its coverage and its regimes.
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


# ---------------------------------------------------------------------------------------------
# the table family: what its draws hold, on the references and tests/ctx_plan_ref.py alone
# ---------------------------------------------------------------------------------------------
TABLE_SEEDS = range(fs.TABLE_SEEDS)
TABLE_TIMES = {}
BEHIND = ("subpixel", "uniqueness", "speckle", "vote", "adjust", "wmf")


@functools.lru_cache(maxsize=None)
def _table_case(seed):
    return fs.table_composition(seed)


@functools.lru_cache(maxsize=None)
def _table_reference(seed):
    import oracle
    oracle.build()
    t = time.perf_counter()
    with np.errstate(all="ignore"):
        e = fs.table_reference(_table_case(seed), oracle)
    TABLE_TIMES[seed] = time.perf_counter() - t
    return e


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _plan(c):
    import ctx_plan_ref
    o = c["opt"]
    return ctx_plan_ref.pair(fs.table_settings(c), c["w"], c["h"], c["D"], c["ch"] if c["entry"] == "rgb" else 0, c["dminl"],
                             c["dminr"], o["volumes"], o["volumes"], False)


def test_every_table_draw_is_the_same_twice_and_accepted_with_the_plan_the_chain_assumes():
    for seed in TABLE_SEEDS:
        c, again = fs.table_composition(seed), _table_case(seed)
        assert c["text"] == again["text"] and c["opt"] == again["opt"] and c["order"] == again["order"], seed
        assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(c["rgb"], again["rgb"])), seed
        assert (c["w"], c["h"], c["D"]) == tuple(fs.table_setup()[k] for k in "whD")          # one context serves them all
        assert sorted(c["order"]) == list(range(len(fs.TABLE_SETTERS)))
        o, s = c["opt"], fs.table_settings(c)
        assert not fs.table_refusals(c), (seed, c["text"])
        chain, need, walker = _plan(c)
        assert not chain.refused(), (seed, c["text"], [(k, st) for cond, k, st in chain.refusals if cond])
        # the plan is what table_reference assumed: the stages that run, where the winners come from, which volumes exist
        for k in ("sgm", "cgf", "cross", "so", "cscale", "perm", "bp", "pm", "subpix", "uniq", "speckle", "vote", "adjust"):
            assert bool(need[k]) == s[k], (seed, k)
        assert bool(need["census"]) == (o["cost"] != "reference"), seed
        assert bool(walker) == (o["family"] in ("guided", "guided+cross_scale", "guided+permeability")), seed
        e = _table_reference(seed)
        assert ("aggl" in e) == ("costl" in e) == (not s["pm"]) and (e["st"] is None) == s["pm"], seed
        assert not o["volumes"] or (need["cost"] and need["agg"] and not s["pm"]), seed
        assert not (s["adjust"] or s["cscale"] or s["perm"]) or need["agg"], seed          # (the stages that read the volume)
        for k, on in (("unique", s["uniq"]), ("margin", s["uniq"]), ("despeckled", s["speckle"]), ("voted", s["vote"]),
                      ("adjusted", s["adjust"]), ("refined", bool(o["wmf"])), ("subpixl", s["subpix"] or s["pm"]),
                      ("subpix_filled", s["subpix"] or s["pm"]), ("mi_table", o["cost"] == "mi"), ("pm_planes", s["pm"])):
            assert (k in e) == on, (seed, k)
    assert fs.table_composition(0, base=7)["text"] != fs.table_composition(0)["text"]


def test_the_table_of_exclusions_is_the_plan_reference_s():
    """every two settings on together, nothing else: TABLE_EXCLUDES names the pair exactly when ctx_plan_ref.pair has a conflict"""
    import ctx_plan_ref
    s0 = fs.table_setup()
    names = [k for k in fs.table_settings(_table_case(0)) if k != "adc_colour"]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            s = dict({k: False for k in names}, adc_colour=False, **{a: True, b: True})
            chain, _, _ = ctx_plan_ref.pair(s, s0["w"], s0["h"], s0["D"], 3, -3, 0, False, False, False)
            conflict = any(bool(cond) for cond, kind, _ in chain.refusals if kind == "conflict")
            assert conflict == bool(fs.table_excluded(s)), (a, b)
    # and what the entry and the volumes add
    for s_on, channels, volumes, kind in ((("cgf",), 0, False, "entry"), (("adcensus", "adc_colour"), 0, False, "entry"),
                                           (("pm",), 3, True, "pm_out")):
        s = dict({k: False for k in names + ["adc_colour"]}, **{k: True for k in s_on})
        chain, _, _ = ctx_plan_ref.pair(s, s0["w"], s0["h"], s0["D"], channels, -3, 0, volumes, volumes, False)
        assert [k for cond, k, _ in chain.refusals if cond] == [kind], s_on


def test_the_table_walk_covers_every_accepted_pair_and_every_option_both_ways():
    cases = [_table_case(s) for s in TABLE_SEEDS]
    pairs = {(c["opt"]["family"], c["opt"]["cost"]) for c in cases}
    assert pairs == {(f, k) for f in fs.TABLE_FAMILIES for k in fs.TABLE_COSTS if f != "patchmatch" or k == "reference"}
    assert len(fs.TABLE_FAMILIES) == 12
    assert [(c["opt"]["family"], c["opt"]["cost"], c["entry"], c["opt"]["volumes"]) for c in cases] == list(fs.TABLE_WALK)
    for k in BEHIND:
        on = sum(bool(c["opt"][k]) for c in cases)
        assert on >= 5 and len(cases) - on >= 5, (k, on)
    assert len({c["opt"]["subpixel"] for c in cases}) == 3 == len({c["opt"]["wmf"] for c in cases})
    free = [c for c in cases if not fs.FAMILIES[c["opt"]["family"]][1] and c["opt"]["cost"] != "adcensus colour"]
    assert 3 * sum(c["entry"] == "rgb" for c in free) >= len(free)
    assert all(c["entry"] == "rgb" for c in cases if c not in free)
    for fam in fs.TABLE_FAMILIES:
        mine = [c for c in cases if c["opt"]["family"] == fam]
        if not fs.FAMILIES[fam][1]:
            assert {c["entry"] for c in mine} == {"gray", "rgb"}, fam
        if fam != "patchmatch":
            assert {c["opt"]["volumes"] for c in mine} == {False, True}, fam
    assert {c["ch"] for c in cases} == {3, 4}
    assert 4 * sum(0 < c["opt"]["bound"] < c["D"] for c in cases) >= len(cases)
    inits = [c["opt"]["mi"]["init"] for c in cases if c["opt"]["mi"]]
    assert inits.count(0) >= 2 and inits.count(1) >= 2 and {c["opt"]["mi"]["iterations"] for c in cases if c["opt"]["mi"]} == {1, 2}
    # the setters come in many orders; as applied, each of the three setters of the cost comes last of them somewhere, always
    # the one that switches the drawn cost on
    assert len({tuple(c["order"]) for c in cases}) == len(cases)
    last = set()
    for c in cases:
        applied = fs.table_applied_order(c)
        assert sorted(applied) == sorted(fs.TABLE_SETTERS)
        trio = [k for k in applied if k in ("cost", "adcensus", "mi")]
        assert trio[-1] == {"census": "cost", "reference": "cost", "mi": "mi"}.get(c["opt"]["cost"], "adcensus"), c["text"]
        last.add(trio[-1])
    assert last == {"cost", "adcensus", "mi"}


def test_the_table_draws_meet_the_regimes():
    """conditions on the inputs, each in at least two draws: the stages behind the winners have something to do, cross-scale and
    the permeability filter move winners, an MI loop's tables differ, a cross-scale child changes its size_d between seeds"""
    import cgf_ref
    import vote_ref
    met = {k: [] for k in ("vote", "adjust", "uniqueness", "speckle", "cross_scale", "permeability", "mi", "child size_d")}
    before = None
    for seed in TABLE_SEEDS:
        c, e = _table_case(seed), _table_reference(seed)
        o = c["opt"]
        lr = e["occlusion"]
        uq = e["unique"] if o["uniqueness"] else lr
        kept = e["despeckled"] if o["speckle"] else uq
        if o["vote"] and (_bits(e["voted"]) != _bits(kept)).any() and not vote_ref.valid(e["voted"], c["dminl"]).all():
            met["vote"].append(seed)
        if o["adjust"] and (_bits(e["before"]) != _bits(e["adjusted"])).any():
            met["adjust"].append(seed)
        if o["uniqueness"] and (_bits(uq) != _bits(lr)).any() and vote_ref.valid(uq, c["dminl"]).any():
            met["uniqueness"].append(seed)
        if o["speckle"] and (_bits(kept) != _bits(uq)).any():
            met["speckle"].append(seed)
        for k in ("cross_scale", "permeability"):
            if o[k] and (cgf_ref.states(e["plainl"])["z"] != e["st"][0]["z"]).any():
                met[k].append(seed)
        if o["mi"] and len(e["mi_tables"]) > 1 and (e["mi_tables"][0] != e["mi_tables"][1]).any():
            met["mi"].append(seed)
        sizes = e.get("child_size_d")
        if sizes and before and before[0] == seed - 1 and sizes[0] != before[1][0]:
            met["child size_d"].append(seed)
        before = (seed, sizes) if sizes else None
    for k, seeds in met.items():
        assert len(seeds) >= 2, f"{k}: met by the draws {seeds} only; " + "; ".join(_table_case(s)["text"] for s in seeds)


def test_no_table_reference_is_slow():
    for seed in TABLE_SEEDS:
        _table_reference(seed)
        assert TABLE_TIMES[seed] < 2.0, (seed, TABLE_TIMES[seed], _table_case(seed)["text"])
    slow = sorted(TABLE_TIMES, key=TABLE_TIMES.get)[-3:]
    print("the slowest table references:", [(s, round(TABLE_TIMES[s], 2)) for s in slow], "all:",
          round(sum(TABLE_TIMES.values()), 1), "s")
