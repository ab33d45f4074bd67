"""The seeded fuzz of region voting (tests/test_gpu_vote_fuzz.py runs these draws through smx_dev_region_vote) on the numpy
reference alone: no GPU.  In the manner of tests/test_fuzz_scenes_cpu.py: shape, label range, parameters, arms, guide kind, map
kind and the form of the call all come from ONE np.random.default_rng(BASE + seed), through the generators of
tests/fuzz_scenes.py, so a case is named by (BASE, seed).  What the GPU file proves depends on what the seeds hold; this file
asserts that over exactly those seeds.  Where one of these fails, the generator or BASE changes -- never what the kernel is
held to.
"""
import functools
import os
import time

import numpy as np
import pytest

import cross_ref
import fuzz_scenes as fs
import vote_ref as ref

F32 = np.float32
BASE = 52120          # (chosen so that the reference meets the conditions below over the twelve seeds)
SEEDS = range(fs.SEEDS)
TILE = ((64,), (4,))            # columns, rows of the voting kernel's tile (smx_vote_geometry; tests/test_gpu_vote.py pins it)
TIMES = {}


def draw(seed, base=BASE):
    rng = np.random.default_rng(int(base) + int(seed))
    w, h = fs.dim(rng, TILE[0], 1, 200), fs.dim(rng, TILE[1] + (64,), 1, 90)
    h = max(1, min(h, 9000 // w))
    D = int(rng.integers(1, 41)) if rng.random() < 0.75 else int(rng.choice([63, 64, 65, 129, 256, 512]))
    dmin = int(-rng.integers(0, 2 * D + 4))
    vote = dict(tau_s=int(rng.choice([0, 3, 20, 60])), tau_h_pct=int(rng.choice([0, 20, 40, 70, 99])),
                iterations=int(rng.integers(0, 9)), interpolate_=int(rng.integers(0, 2)))
    l1 = 63 if rng.random() < 0.25 else int(rng.integers(1, 40))
    tau1 = int(rng.choice([6, 12, 20, 40, 256]))
    arms = dict(l1=l1, l2=int(rng.integers(0, l1 + 1)), tau1=tau1, tau2=int(rng.integers(1, tau1 + 1)))
    ch = int(rng.choice([1, 3, 4]))
    guide = fs.image(rng, seed % 4, w, h, ch)
    disp = fs.disparity(rng, seed, w, h, dmin, D)
    sparse = rng.random() < 0.25            # a few voters in a void: long rays, and outliers that no ray helps
    keep = rng.random((h, w)) < 0.004
    if sparse:
        disp = np.where(keep, disp, F32(dmin - 100)).astype(F32)
    # the right map: the labels of the mirrored range with the same kinds of holes and messy values, or none
    right = None if rng.random() < 0.25 else (-fs.disparity(rng, seed + 1, w, h, dmin, D)).astype(F32)
    d_lr = int(rng.integers(0, 3))
    form = dict(in_place=bool(rng.integers(0, 2)), misalign=int(rng.choice([0, 1, 255])))
    return dict(w=w, h=h, D=D, dmin=dmin, vote=vote, arms=arms, ch=ch, guide=guide, disp=disp, right=right, d_lr=d_lr, form=form,
                text=f"{w}x{h} labels [{dmin},{dmin + D}) {fs.KINDS[seed % 4]} ch {ch} vote {vote['tau_s']},{vote['tau_h_pct']},"
                     f"{vote['iterations']} interpolate {vote['interpolate_']} arms {l1},{arms['l2']} tau {tau1},{arms['tau2']} "
                     f"right {'none' if right is None else 'given'} d_lr {d_lr} {'in place' if form['in_place'] else 'out of place'} "
                     f"misalign {form['misalign']}{' messy' if seed % 3 == 0 else ''}{' sparse' if sparse else ''}")


def accepted(c):
    """the argument checks of smx_dev_region_vote and smx_dev_cross_arms on the drawn case"""
    v = c["vote"]
    return ref.shape_ok(c["w"], c["h"], c["D"]) and ref.params_ok(v["tau_s"], v["tau_h_pct"], v["iterations"], v["interpolate_"]) and \
        cross_ref.params_ok(iterations=1, **c["arms"]) and c["ch"] in (1, 3, 4) and c["disp"].shape == (c["h"], c["w"]) and \
        c["disp"].dtype == F32 and (c["right"] is None or (c["right"].shape == c["disp"].shape and c["right"].dtype == F32))


@functools.lru_cache(maxsize=None)
def reference(seed, base=BASE):
    """(case, packed arms, expected map, stats, pixels filled in a round after the first)"""
    c = draw(seed, base)
    t = time.perf_counter()
    a = cross_ref.arms(c["guide"], **c["arms"])
    t_arms = time.perf_counter() - t
    v = c["vote"]
    stats, rounds = {}, []
    m = ref.vote(c["disp"], a, c["dmin"], c["D"], v["tau_s"], v["tau_h_pct"], v["iterations"], stats, rounds)
    want = ref.interpolate(m, c["guide"], c["right"], c["dmin"], c["D"], c["d_lr"], stats) if v["interpolate_"] else m
    TIMES[seed] = time.perf_counter() - t - t_arms             # (the arms are cross_ref's: tests/test_fuzz_scenes_cpu.py times them)
    late = int((rounds[-1].view(np.uint32) != rounds[0].view(np.uint32)).sum()) if len(rounds) > 1 else 0
    want.setflags(write=False)
    return c, cross_ref.pack_arms(a), want, stats, late


def test_every_draw_is_inside_the_contract_and_the_same_twice():
    for seed in SEEDS:
        c, again = draw(seed), draw(seed)
        assert accepted(c), (seed, c["text"])
        assert c["text"] == again["text"]
        for k in ("guide", "disp", "right"):
            assert (c[k] is None and again[k] is None) or c[k].tobytes() == again[k].tobytes(), (seed, k)
    assert draw(0, base=7)["text"] != draw(0)["text"]


def test_the_gpu_file_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_vote_fuzz.py")).read()
    for word in ("pytest.skip", "importorskip", "skipif", "xfail"):
        assert word not in src, word


def test_no_reference_call_is_slow():
    for seed in SEEDS:
        reference(seed)
        assert TIMES[seed] < 2.0, (seed, TIMES[seed], draw(seed)["text"])


def test_the_seeds_hold_every_regime():
    """an accepted vote, a rejection by tau_s alone and one by tau_h_pct alone, a pixel filled only in a round after the first,
    an interpolated occlusion, an interpolated mismatch and an outlier with no candidate"""
    total, late = {}, 0
    for seed in SEEDS:
        _, _, _, stats, l = reference(seed)
        late += l
        for k, v in stats.items():
            total[k] = total.get(k, 0) + v
    print("over the seeds:", total, "filled after the first round:", late)
    for k in ("accepted", "reject_s", "reject_h", "occlusion", "mismatch", "no_candidate"):
        assert total.get(k, 0) > 0, (k, total)
    assert late > 0


def test_the_seeds_hold_every_form_of_the_call():
    cs = [draw(s) for s in SEEDS]
    assert {c["form"]["in_place"] for c in cs} == {False, True} and {c["form"]["misalign"] for c in cs} == {0, 1, 255}
    assert {c["ch"] for c in cs} == {1, 3, 4} and any(c["right"] is None for c in cs) and any(c["right"] is not None for c in cs)
    assert {c["vote"]["interpolate_"] for c in cs} == {0, 1} and any(c["D"] > 64 for c in cs) and any(c["D"] <= 64 for c in cs)
    assert any(c["vote"]["iterations"] == 0 for c in cs) or any(c["vote"]["iterations"] >= 5 for c in cs)
    edges = set(fs.edge_list(TILE[0], 1, 200))
    assert any(c["w"] in edges for c in cs) and any(c["w"] not in edges for c in cs) and any(c["w"] > 64 for c in cs)
    assert any(c["h"] > 4 for c in cs)
    assert any(np.isnan(c["disp"]).any() for c in cs)


def test_the_results_differ_from_the_inputs():
    changed = sum(int((reference(s)[2].view(np.uint32) != draw(s)["disp"].view(np.uint32)).any()) for s in SEEDS)
    assert changed >= 6, changed
