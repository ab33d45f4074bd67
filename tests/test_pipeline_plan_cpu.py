"""PairPipeline's and ShardedPair's rules -- what a constructor call refuses, and what an accepted one owns and how large --
against the constructors as they stood before they had a stage table (tests/pipeline_plan_ref.py), without a GPU.

plan_pipeline() (stereo_matching_cuda_amd/pipeline_plan.py) plans and allocates nothing, and the workspace queries it asks are
host functions of the built library, so every point is walked here: for every point the verdict must equal the reference's; an
accepted point must equal it in every option, byte count, buffer (shape, dtype, zeroed) and cross-scale level; a refused point
may name another refusal than the old constructor did where several apply, so its message is held to this: it is of the kind
of, and names every keyword of, a refusal that the reference lists for that point.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k pipeline_plan
"""
import ctypes as C
import inspect
import itertools
import re

import numpy as np
import pytest

import ctx_plan_ref
import pipeline_plan_ref as ref
import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, pipeline_plan as pp

W, H, D = 33, 9, 5
HUGE = 1 << 62
AGGS = (None, "sgm", "bp", "cross", "scanline", "cross-scanline", "patchmatch", "bogus")
COSTS = (None, "census", "adcensus", "mi", "bogus")
# the phrase that tells a message's kind, the first that is found
KINDS = (("sharded", "not part of the sharded driver"), ("world", "world == 1"), ("budget", "max_ws_bytes"),
         ("conflict", " does not run with "), ("slices", "no slice sub-range"), ("shape", " does not take "),
         ("level", "narrower than 2 pixels"), ("belongs", " belongs to "), ("value", " must be "), ("range", " needs "))


@pytest.fixture(scope="module")
def lib():
    return smx.lib()


def plain(v):
    """A value of a plan as something that compares: a struct by its type and bytes."""
    if isinstance(v, C.Structure):
        return type(v).__name__, bytes(v)
    if isinstance(v, dict):
        return {k: plain(x) for k, x in v.items()}
    return v


def outcome(plan):
    """A PipelinePlan in the form of the reference's outcome."""
    buffers = dict.fromkeys(pp.BUFFERS)
    for name, shape, dtype, zeroed in plan.buffers:
        assert name in buffers and buffers[name] is None, name
        buffers[name] = (tuple(shape), dtype, bool(zeroed))
    buffers["cs_gray"] = [(gray, "uint8", False) for _, _, gray, _ in plan.levels]
    buffers["cs_rgb"] = [(rgb, "uint8", False) if rgb else None for _, _, _, rgb in plan.levels]
    levels = [dict(handed=plain(handed), shares=pp.LEVEL_SHARES, outcome=outcome(sub)) for handed, sub, _, _ in plan.levels]
    assert plan.slices_in_flight == plan.options["slices_in_flight"]
    return dict(options=plain(plan.options), bytes=dict(plan.bytes), buffers=buffers, levels=levels)


def ref_outcome(out):
    return dict(options=plain(out["options"]), bytes=out["bytes"], buffers=out["buffers"],
                levels=[dict(handed=plain(lv["handed"]), shares=lv["shares"], outcome=ref_outcome(lv["outcome"])) for lv in out["levels"]])


def kind_of(msg):
    return next(kind for kind, phrase in KINDS if phrase in msg)


def listed(msg, refusals):
    kind = kind_of(msg)
    return any(k == kind and all(re.search(rf"\b{kw}\b", msg) for kw in kws) for kws, k in refusals)


def check(lib, geometry=(W, H, D), sharded=None, **kw):
    """One point: plan_pipeline (or, with sharded=(rank, world), ShardedPair's rules and then the plan) against the reference.
    -> the reference's verdict and outcome."""
    if sharded is None:
        verdict, want = ref.pipeline(lib, *geometry, **kw)
    else:
        verdict, want = ref.sharded(lib, *geometry, rank=sharded[0], world=sharded[1], **kw)
    try:
        if sharded is not None:
            msg = pp.sharded_refusal(sharded[1], kw)
            if msg:
                raise ValueError(msg)
            s0, s1 = ref.shard_range(geometry[2], *sharded)
            kw = dict(kw, s_begin=s0, s_end=s1)
        plan = pp.plan_pipeline(lib, *geometry, **kw)
    except ValueError as e:
        assert type(e) is ValueError
        assert verdict == "refused", (kw, str(e))
        assert listed(str(e), want), (kw, str(e), want)
        return verdict, want
    assert verdict == "ok", (kw, want)
    got, want_plain = outcome(plan), ref_outcome(want)
    for part in ("options", "bytes", "buffers", "levels"):
        assert got[part] == want_plain[part], (kw, part, got[part], want_plain[part])
    return verdict, want


def grid():
    """The full product of every option that takes part in an exclusion, a slice-range rule or the budget."""
    for agg, cost, guidance, cscale, perm, adjust, uniq, subpix, want_agg, sub, mk in itertools.product(
            AGGS, COSTS, (None, "rgb"), (None, True), (None, True), (None, True), (None, 0.25), (None, "parabola"), (False, True),
            (False, True), (False, True)):
        kw = dict(aggregation=agg, cost=cost, guidance=guidance, cross_scale=cscale, permeability=perm, adjust=adjust, uniqueness=uniq,
                  subpixel=subpix, want_agg=want_agg, multi_kernel=mk)
        if sub:
            kw.update(s_begin=1, s_end=4)
        yield kw


def test_every_point_of_the_grid_plans_and_refuses_as_the_old_constructor_did(lib):
    seen = {"ok": 0, "refused": 0}
    first = {}
    for kw in grid():
        verdict, want = check(lib, slices_in_flight=2, **kw)
        seen[verdict] += 1
        if verdict == "refused":
            first[want[0]] = first.get(want[0], 0) + 1
    assert seen["ok"] + seen["refused"] == len(AGGS) * len(COSTS) * 2 ** 9
    assert 0 < seen["ok"] < seen["refused"]                     # (most combinations are refused)
    # every kind of refusal the grid can reach was what the old constructor reported somewhere
    assert {kind for _, kind in first} == {"value", "conflict", "slices"}


def test_the_options_that_exclude_nothing_cross_with_the_rest(lib):
    """speckle, vote and wmf, each value and together, against every single option of the grid and every aggregation x cost."""
    base = dict(aggregation=None, cost=None, guidance=None, cross_scale=None, permeability=None, adjust=None, uniqueness=None,
                subpixel=None, want_agg=False, multi_kernel=False)
    one_at_a_time = [dict(base, **{k: v}) for k, vs in (
        ("aggregation", AGGS), ("cost", COSTS), ("guidance", ("rgb",)), ("cross_scale", (True,)), ("permeability", (True,)),
        ("adjust", (True,)), ("uniqueness", (0.25,)), ("subpixel", ("parabola", "equiangular")), ("want_agg", (True,)),
        ("multi_kernel", (True,))) for v in vs]
    one_at_a_time += [dict(p, s_begin=1, s_end=4) for p in one_at_a_time]
    products = [dict(base, aggregation=a, cost=c) for a in AGGS for c in COSTS]
    ok = 0
    for speckle, vote, wmf in itertools.product((None, True, smx.default_speckle_params()), (None, True, smx.default_vote_params()),
                                                (None, "occluded", "all", "bogus")):
        for kw in one_at_a_time + products:
            ok += check(lib, speckle=speckle, vote=vote, wmf=wmf, **kw)[0] == "ok"
    assert ok > 100
    # the parameters that go with them, with and without their stage
    arms = smx.default_cross_params()
    arms.iterations = 3
    for kw in (dict(vote=True, vote_arms=arms), dict(wmf="all", wmf_params=smx.default_wmf_params()), dict(wmf_params=smx.default_wmf_params()),
               dict(census_params=smx.default_census_params()), dict(cost="census", census_params=smx.default_census_params()),
               dict(adcensus_params=smx.default_adcensus_params()), dict(cost="adcensus", adcensus_params=smx.default_adcensus_params()),
               dict(sgm_params=smx.default_sgm_params()), dict(aggregation="sgm", sgm_params=smx.default_sgm_params()),
               dict(cross_params=smx.default_cross_params()), dict(aggregation="cross-scanline", cross_params=smx.default_cross_params(),
                                                                   scanline_params=smx.default_scanline_params())):
        assert check(lib, **kw)[0] == "ok", kw
    plan = pp.plan_pipeline(lib, W, H, D, vote=True, vote_arms=arms)
    assert plan.options["vote_arms"].iterations == 1 and arms.iterations == 3         # (a copy: the caller's struct is not written)


def test_params_without_their_stage_and_wrong_typed_values_are_refused(lib):
    belonging = dict(pm_params=smx.default_pm_params(), bp_params=smx.default_bp_params(), scanline_params=smx.default_scanline_params(),
                     mi_params=smx.default_mi_params(), vote_arms=smx.default_cross_params())
    for name, value in belonging.items():
        for agg in (None, "sgm", "cross"):
            verdict, want = check(lib, aggregation=agg, **{name: value})
            assert verdict == "refused" and want[0][1] == "belongs" and want[0][0][0] == name
        assert check(lib, sharded=(0, 1), **{name: value})[0] == "refused"
    for kw in (dict(adjust="yes"), dict(vote=smx.default_cross_params()), dict(vote=False), dict(speckle=1), dict(permeability=32.0),
               dict(cross_scale=4), dict(cross_scale=smx.default_perm_params()), dict(vote=True, vote_arms=smx.default_vote_params()),
               dict(vote_arms="arms"), dict(aggregation="patchmatch", pm_params=smx.default_bp_params()), dict(uniqueness="much"),
               dict(subpixel="cubic"), dict(subpixel=True), dict(wmf=True), dict(guidance="gray"), dict(guidance=True), dict(cost=1),
               dict(aggregation="SGM"), dict(permeability=smx.default_adjust_params()), dict(speckle=smx.default_vote_params())):
        verdict, want = check(lib, **kw)
        assert verdict == "refused" and want[0][1] == "value", (kw, want)


def _bp(**kw):
    p = smx.default_bp_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _set(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_every_limit_at_and_just_past_it(lib):
    """[(what is asked, whether it is taken)]: the reference decides, and the limit lies where the issue of record says."""
    big = 1 << 20
    inf, nan = float("inf"), float("nan")
    cases = []
    for agg in ("sgm", "bp", "scanline", "cross-scanline"):
        cases += [(dict(geometry=(16, 8, d), aggregation=agg), d == 256) for d in (256, 257)]
    for stage in ("adjust", "vote"):
        cases += [(dict(geometry=(16, 8, d), **{stage: True}), d == 512) for d in (512, 513)]
    cases += [(dict(geometry=(1, hh, 4), guidance="rgb"), hh == 65535) for hh in (65535, 65536)]
    # w*h at 2^31 - 1 (a prime: one row or one column) and at 2^31, for every stage whose query has the bound
    for kw in (dict(guidance="rgb"), dict(aggregation="sgm"), dict(aggregation="bp"), dict(aggregation="cross"), dict(aggregation="scanline"),
               dict(aggregation="cross-scanline"), dict(adjust=True), dict(vote=True), dict(permeability=True)):
        cases += [(dict(geometry=((1 << 31) - 1, 1, 1), max_ws_bytes=HUGE, **kw), True),
                  (dict(geometry=(1 << 30, 2, 1), max_ws_bytes=HUGE, **kw), False)]
    cases += [(dict(geometry=(1, (1 << 31) - 1, 1), max_ws_bytes=HUGE, aggregation="patchmatch"), True),
              (dict(geometry=(2, 1 << 30, 1), max_ws_bytes=HUGE, aggregation="patchmatch"), False)]
    for dl, dr, ok in ((-big, 0, True), (-big - 1, 0, False), (big, big, True), (0, big + 1, False), (0, -big, True), (0, -big - 1, False)):
        cases.append((dict(geometry=(16, 8, 4), aggregation="patchmatch", dminl=dl, dminr=dr), ok))
    cases += [(dict(geometry=(ww, 1, 4), aggregation="patchmatch", max_ws_bytes=HUGE), ww < 1 << 24) for ww in ((1 << 24) - 1, 1 << 24)]
    # the parameter ranges' edges
    cases += [(dict(aggregation="bp", bp_params=_bp(step=s)), 0 <= s <= 4095) for s in (0, 4095, 4096, -1)]
    cases += [(dict(aggregation="bp", bp_params=_bp(levels=n)), 1 <= n <= 8) for n in (0, 1, 8, 9)]
    cases += [(dict(aggregation="bp", bp_params=_bp(data_scale=s)), 0 < s < inf) for s in (0.0, 0.5, inf)]
    cases += [(dict(aggregation="patchmatch", pm_params=_set(smx.default_pm_params(), radius=r)), 0 <= r <= 17) for r in (-1, 0, 17, 18)]
    cases += [(dict(aggregation="patchmatch", pm_params=_set(smx.default_pm_params(), iterations=n)), 1 <= n <= 16) for n in (0, 1, 16, 17)]
    cases += [(dict(aggregation="patchmatch", pm_params=_set(smx.default_pm_params(), max_slope=s)), 0 <= s <= 8) for s in (0.0, 8.0, 8.5)]
    cases += [(dict(cross_scale=_set(smx.default_cscale_params(), scales=n)), 1 <= n <= 5) for n in (0, 1, 5, 6)]
    cases += [(dict(cross_scale=_set(smx.default_cscale_params(), lambda_=v)), 0 <= v < inf) for v in (-0.5, 0.0, inf)]
    cases += [(dict(adjust=_set(smx.default_adjust_params(), tau_e=t)), 1 <= t <= 512) for t in (0, 1, 512, 513)]
    cases += [(dict(adjust=_set(smx.default_adjust_params(), iterations=n)), 1 <= n <= 8) for n in (0, 1, 8, 9)]
    cases += [(dict(adjust=_set(smx.default_adjust_params(), vertical=v)), v in (0, 1)) for v in (0, 1, 2)]
    cases += [(dict(permeability=_set(smx.default_perm_params(), sigma=s)), 0 < s < inf) for s in (0.0, 1e-3, inf, nan)]
    cases += [(dict(uniqueness=u), 0 < u < inf) for u in (0, 0.0, 1e-6, 3, inf, nan, -1.0)]
    cases += [(dict(cost="mi", mi_params=_set(smx.default_mi_params(), iterations=n)), 1 <= n <= 16) for n in (0, 1, 16, 17)]
    cases += [(dict(cost="mi", mi_params=_set(smx.default_mi_params(), init=i)), i in (0, 1)) for i in (0, 1, 2)]
    for kw, ok in cases:
        verdict, want = check(lib, **kw)
        assert (verdict == "ok") == bool(ok), (kw, want if verdict == "refused" else None)
    # a cross-scale pyramid whose coarsest level is 1 and 2 pixels wide
    two = _set(smx.default_cscale_params(), scales=2)
    widths = {}
    for ww in range(2, 8):
        widths.setdefault(pp.cscale_level(lib, ww, H, 0, D, 1)[0], ww)
    assert {1, 2} <= set(widths)
    for cost, guidance in ((None, None), ("adcensus", "rgb"), ("mi", None)):
        verdict, want = check(lib, geometry=(widths[1], H, D), cross_scale=two, cost=cost, guidance=guidance)
        assert verdict == "refused" and want == [(("cross_scale",), "level")]
        assert check(lib, geometry=(widths[2], H, D), cross_scale=two, cost=cost, guidance=guidance)[0] == "ok"
    # ... and one of every depth, with each cost and guide a level is handed, a colour AD term among them
    colour = _set(smx.default_adcensus_params(), colour=1)
    for scales, (cost, guidance), adjust in itertools.product((1, 2, 3, 4, 5), ((None, None), ("census", None), ("adcensus", "rgb"), ("mi", None),
                                                                                 ("adcensus", None)), (None, True)):
        kw = dict(cross_scale=_set(smx.default_cscale_params(), scales=scales), cost=cost, guidance=guidance, adjust=adjust,
                  adcensus_params=colour if cost == "adcensus" and guidance is None else None, max_ws_bytes=1 << 20)
        verdict, want = check(lib, **kw)
        assert verdict == "ok" and len(want["levels"]) == scales - 1, kw


def test_the_budget(lib):
    n = W * H
    volumes = 2 * D * n * 4
    # every budgeted stage at exactly what the reference says it needs, and at one byte less
    for kw, name, holds in ((dict(adjust=True), "adjust_ws_bytes", volumes), (dict(aggregation="sgm"), "sgm_ws_bytes", volumes),
                            (dict(aggregation="bp"), "bp_ws_bytes", volumes), (dict(aggregation="scanline"), "so_ws_bytes", volumes),
                            (dict(aggregation="patchmatch"), "pm_ws_bytes", 8 * n * 4)):
        need = check(lib, **kw)[1]["bytes"][name] + holds
        verdict, want = check(lib, max_ws_bytes=need, **kw)
        # (what adjust and the optimiser hold is taken off what the slices in flight may use; what semi-global matching, belief
        # propagation and PatchMatch stereo hold is not, and they run no chunks)
        assert verdict == "ok" and (want["options"]["slices_in_flight"] == 1 or kw.get("aggregation") in ("sgm", "bp", "patchmatch")), kw
        verdict, want = check(lib, max_ws_bytes=need - 1, **kw)
        assert verdict == "refused" and want[0][1] == "budget", kw
    # the chain holds its cross stage beside the optimiser: it does not fit what the optimiser alone needs, and the smallest
    # budget it fits leaves the cross stage one slice in flight
    need = check(lib, aggregation="cross-scanline")[1]["bytes"]["so_ws_bytes"] + volumes
    lo, hi = need, need + (1 << 30)
    assert ref.pipeline(lib, W, H, D, aggregation="cross-scanline", max_ws_bytes=hi)[0] == "ok"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ref.pipeline(lib, W, H, D, aggregation="cross-scanline", max_ws_bytes=mid)[0] == "ok" else (mid, hi)
    for budget, ok in ((need - 1, False), (need, False), (lo, False), (hi, True)):
        for cost in (None, "census"):
            verdict, want = check(lib, aggregation="cross-scanline", cost=cost, max_ws_bytes=budget)
            if cost is None:
                assert (verdict == "ok") == ok and (ok or want[0][1] == "budget")
                assert not ok or (want["options"]["slices_in_flight"] == 1 and want["buffers"]["_so_chunk"] is not None)
    # the slices in flight: 7 labels halve to 4, 2 and 1; every budget at which a path's count changes, and one byte less
    for kw in (dict(), dict(multi_kernel=True), dict(cost="census"), dict(cost="mi", want_agg=True), dict(guidance="rgb"),
               dict(guidance="rgb", cost="adcensus", want_agg=True), dict(aggregation="cross"), dict(aggregation="cross", cost="census"),
               dict(aggregation="cross", want_agg=True), dict(s_begin=0, s_end=7), dict(aggregation="sgm"), dict(permeability=True), dict(aggregation="scanline"),
               dict(aggregation="cross-scanline"), dict(aggregation="cross-scanline", cost="adcensus", want_agg=True),
               dict(aggregation="scanline", adjust=True), dict(aggregation="bp", cost="census"), dict(adjust=True, guidance="rgb")):
        kw = dict(dict(geometry=(W, H, 7) if "s_end" not in kw else (W, H, 9)), **kw)
        seen = set()
        top = 1 << 24
        assert check(lib, max_ws_bytes=top, **kw)[1]["options"]["slices_in_flight"] == 7
        edges = []
        for sif in (7, 4, 2):
            # the smallest budget that still gives `sif` slices, by the reference
            lo, hi = 0, top
            while hi - lo > 1:
                mid = (lo + hi) // 2
                v, out = ref.pipeline(lib, *kw["geometry"], **{k: x for k, x in kw.items() if k != "geometry"}, max_ws_bytes=mid)
                lo, hi = (lo, mid) if v == "ok" and out["options"]["slices_in_flight"] >= sif else (mid, hi)
            edges += [hi, hi - 1]
        for budget in edges + [0, 1, top]:
            verdict, want = check(lib, max_ws_bytes=budget, **kw)
            if verdict == "ok":
                seen.add(want["options"]["slices_in_flight"])
        # (belief propagation holds more than the walker's workspace for 4 slices, and does not deduct it: below that it is refused)
        assert seen == ({7, 4} if kw.get("aggregation") == "bp" else {7, 4, 2, 1}), (kw, seen)
    for sif in (None, 0, 1, 3, 7, 100):
        assert check(lib, geometry=(W, H, 7), slices_in_flight=sif, want_agg=True, cost="census")[0] == "ok"
    # adjust in front of the scan-line optimiser: both deductions
    out = check(lib, adjust=True, aggregation="scanline")[1]["bytes"]
    need = out["adjust_ws_bytes"] + volumes + out["so_ws_bytes"] + volumes
    for budget in (need, need - 1, need - out["so_ws_bytes"] - volumes, need - out["so_ws_bytes"] - volumes - 1):
        check(lib, adjust=True, aggregation="scanline", max_ws_bytes=budget)
        check(lib, adjust=True, aggregation="cross-scanline", max_ws_bytes=budget + (1 << 16))
    assert check(lib, adjust=True, aggregation="scanline", max_ws_bytes=need)[0] == "ok"
    assert check(lib, adjust=True, aggregation="scanline", max_ws_bytes=need - 1)[1][0] == (("aggregation",), "budget")
    assert check(lib, adjust=True, aggregation="scanline", max_ws_bytes=out["adjust_ws_bytes"] + volumes - 1)[1][0] == (("adjust",), "budget")
    # (what a cross-scale level is handed is what adjust left)
    verdict, want = check(lib, adjust=True, cross_scale=True, max_ws_bytes=1 << 22)
    assert want["levels"][0]["handed"]["max_ws_bytes"] == (1 << 22) - out["adjust_ws_bytes"] - volumes


def test_the_sharded_driver_reads_the_same_rules(lib):
    """ShardedPair's refusals over every row alone and the grid's exclusion options, on one rank and on each of three."""
    singles = [dict()] + [dict(aggregation=a) for a in AGGS[1:]] + [dict(cost=c) for c in COSTS[1:]] + [
        dict(guidance="rgb"), dict(cross_scale=True), dict(permeability=True), dict(adjust=True), dict(uniqueness=0.25),
        dict(subpixel="parabola"), dict(speckle=True), dict(vote=True), dict(wmf="all"), dict(want_agg=True),
        dict(uniqueness=0.25, wmf="occluded", want_agg=True, guidance="rgb"), dict(aggregation="cross", cost="census"),
        dict(subpixel="equiangular", speckle=True)]
    taken = 0
    for kw in singles:
        for rank, world in ((0, 1), (0, 3), (1, 3), (2, 3), (0, 8)):
            taken += check(lib, sharded=(rank, world), **kw)[0] == "ok"
    assert taken == 5 + 5 * 3 + 1 + 1 + 1       # nothing on, the colour guide, wmf and want_agg anywhere; uniqueness, subpixel and the mix on one rank
    # what the old list called by the wrong name keeps its refusal and gets its own
    assert "cross-based aggregation is not part of the sharded driver" in pp.sharded_refusal(1, dict(aggregation="cross"))
    for row in pp.STAGES:
        on = {row.kw: row.values[0] if row.values else True}
        msg = pp.sharded_refusal(1, on)
        assert (msg is None) == row.sharded and (msg is None or (row.noun in msg and row.kw in msg)), row.key


def test_the_exclusions_agree_with_the_persistent_context(lib):
    """Whole-range pipelines without wmf and without caller's volumes against ctx_plan_ref.pair on the corresponding settings:
    "some two stages do not run together" must be the same verdict on both sides over the whole grid."""
    # every disagreement that is on purpose, as (pipeline keywords, why); DESIGN.md §4.3t carries the same list
    ON_PURPOSE = []
    differ = []
    for kw in grid():
        if "s_begin" in kw or kw["multi_kernel"] or "bogus" in (kw["aggregation"], kw["cost"]) or kw["cost"] == "mi":
            continue                    # (the context's mutual-information row has a walk of its own, test_ctx_plan_mi_cpu.py)
        for speckle, vote in ((None, None), (True, True)):
            agg = kw["aggregation"]
            s = dict(census=kw["cost"] == "census", adcensus=kw["cost"] == "adcensus", adc_colour=False, sgm=agg == "sgm",
                     cgf=kw["guidance"] == "rgb", cross=agg in ("cross", "cross-scanline"), so=agg in ("scanline", "cross-scanline"),
                     cscale=bool(kw["cross_scale"]), perm=bool(kw["permeability"]), bp=agg == "bp", pm=agg == "patchmatch",
                     adjust=bool(kw["adjust"]), uniq=kw["uniqueness"] is not None, subpix=kw["subpixel"] is not None,
                     speckle=bool(speckle), vote=bool(vote))
            s = {k: np.asarray(v) for k, v in s.items()}
            chain, _, _ = ctx_plan_ref.pair(s, W, H, D, 3 if kw["guidance"] else 0, -(D - 1), 0, wants_cost=np.asarray(False),
                                            wants_agg=np.asarray(kw["want_agg"]), wants_mean=np.asarray(False))
            ctx = any(bool(cond) for cond, kind, _ in chain.refusals if kind in ("conflict", "pm_out"))
            verdict, want = ref.pipeline(lib, W, H, D, speckle=speckle, vote=vote, **kw)
            ours = verdict == "refused" and any(kind == "conflict" for _, kind in want)
            assert verdict == "ok" or all(kind == "conflict" for _, kind in want)
            if ctx != ours:
                differ.append(kw)
    assert differ == [kw for kw, _ in ON_PURPOSE]


def test_the_table_is_symmetric_and_covers_the_constructor():
    from stereo_matching_cuda_amd.device import PairPipeline
    keys = [r.key for r in pp.STAGES]
    assert len(set(keys)) == len(keys) == 19
    for a in keys:
        assert a not in pp.EXCLUDES[a]
        for b, why in pp.EXCLUDES[a].items():
            assert pp.EXCLUDES[b][a] == why and why
    # (6 aggregations x 3 guided-only stages, permeability + cross-scale, PatchMatch + 3 costs + 4 more)
    assert sum(len(v) for v in pp.EXCLUDES.values()) == 2 * (18 + 1 + 7)
    # two values of one keyword are never both on: no exclusion is stated between them
    for a, b in itertools.combinations(pp.STAGES, 2):
        assert not (a.kw == b.kw and b.key in pp.EXCLUDES[a.key])
    # every keyword of the constructor is a row's, a row's *_params, or plain geometry
    rows = {r.kw for r in pp.STAGES} | {r.params_kw for r in pp.STAGES if r.params_kw}
    names = [p for p in inspect.signature(PairPipeline.__init__).parameters if p != "self"]
    assert set(names) == rows | set(pp.GEOMETRY) and not rows & set(pp.GEOMETRY)
    assert [p for p in inspect.signature(pp.plan_pipeline).parameters][:12] == ["lib"] + [g for g in pp.GEOMETRY if g != "device"]
    # a row that is charged against max_ws_bytes has a workspace and says what it holds; a strict *_params names its type or range
    for r in pp.STAGES:
        assert (r.holds is None) == (r.holds_text is None) and (r.holds is None or r.key in pp.WS_BYTES)
        assert (r.range_ok is None) == (r.range_text is None)
        assert not r.limit or r.ws
        if r.default:
            assert isinstance(r.default(), C.Structure)
            assert r.range_ok is None or r.range_ok(r.default()), r.key      # (the defaults lie in their range)
