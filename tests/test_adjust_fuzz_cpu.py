"""The seeded fuzz of the depth-discontinuity adjustment (tests/test_gpu_adjust_fuzz.py runs these draws through
smx_dev_discontinuity_adjust) on the numpy reference alone: no GPU.  In the manner of tests/test_vote_fuzz_cpu.py: shape, label
range, parameters, map kind, volume kind, sub-pixel mode and the form of the call all come from ONE
np.random.default_rng(BASE + seed), through the generators of tests/fuzz_scenes.py, so a case is named by (BASE, seed).  What the
GPU file proves depends on what the seeds hold; this file asserts that over exactly those seeds.  Where one of these fails, the
generator or BASE changes -- never what the kernel is held to.
"""
import functools
import os
import time

import numpy as np

import adjust_ref as ref
import fuzz_scenes as fs
import subpix_ref

F32 = np.float32
BASE = 53140          # (chosen so that the reference meets the conditions below over the twelve seeds)
SEEDS = range(fs.SEEDS)
TILE = ((64,), (4,))            # columns, rows of a workgroup of the round kernel (smx_adjust_geometry; tests/test_gpu_adjust.py pins it)
TIMES = {}


def draw(seed, base=BASE):
    rng = np.random.default_rng(int(base) + int(seed))
    w, h = fs.dim(rng, TILE[0], 1, 200), fs.dim(rng, TILE[1] + (64,), 1, 90)
    D = int(rng.integers(1, 41)) if rng.random() < 0.75 else int(rng.choice([63, 64, 65, 129, 256, 512]))
    h = max(1, min(h, 9000 // w, fs.CELLS // (w * D)))
    dmin = int(rng.integers(-2 * D - 4, 6))
    adjust = dict(tau_e=int(rng.choice([1, 1, 2, 3, D])), vertical=int(rng.integers(0, 2)), iterations=int(rng.integers(1, 9)))
    disp = fs.disparity(rng, seed, w, h, dmin, D)
    vol = fs.volume(rng, fs.volume_kind(seed), D, h, w)
    mode = int(rng.integers(0, 3))             # 0: no sub-pixel map
    sub = rng.normal(size=(h, w)).astype(F32) if mode else None
    form = dict(in_place=bool(rng.integers(0, 2)), misalign=int(rng.choice([0, 1, 255])))
    return dict(w=w, h=h, D=D, dmin=dmin, adjust=adjust, disp=disp, vol=vol, mode=mode, sub=sub, form=form,
                text=f"{w}x{h} labels [{dmin},{dmin + D}) volume {fs.VOLUMES[fs.volume_kind(seed)]} adjust {adjust['tau_e']},"
                     f"{adjust['iterations']} vertical {adjust['vertical']} sub-pixel mode {mode} "
                     f"{'in place' if form['in_place'] else 'out of place'} misalign {form['misalign']}{' messy' if seed % 3 == 0 else ''}")


def accepted(c):
    """the argument checks of smx_dev_discontinuity_adjust on the drawn case"""
    return ref.shape_ok(c["w"], c["h"], c["D"]) and ref.params_ok(**c["adjust"]) and c["disp"].shape == (c["h"], c["w"]) and \
        c["disp"].dtype == F32 and c["vol"].shape == (c["D"], c["h"], c["w"]) and c["vol"].dtype == F32 and \
        c["mode"] in (0, subpix_ref.PARABOLA, subpix_ref.EQUIANGULAR) and (c["sub"] is None) == (c["mode"] == 0)


@functools.lru_cache(maxsize=None)
def reference(seed, base=BASE):
    """(case, expected map, expected sub-pixel map or None, stats)"""
    c = draw(seed, base)
    t = time.perf_counter()
    stats, rounds = {}, []
    a = c["adjust"]
    out = ref.adjust(c["disp"], c["vol"], c["dmin"], mode=c["mode"] or None, sub=c["sub"], stats=stats, rounds=rounds, **a)
    want, wsub = out if c["mode"] else (out, None)
    TIMES[seed] = time.perf_counter() - t
    # pixels that changed in a round after the first, and changed pixels whose final slice is the first / the last of the range
    stats["late"] = int((rounds[-1].view(np.uint32) != rounds[0].view(np.uint32)).sum())
    _, z0 = ref.labelled(c["disp"], c["dmin"], c["D"])
    lab, z1 = ref.labelled(want, c["dmin"], c["D"])
    moved = lab & (z1 != z0)
    stats["to_first"] = int((moved & (z1 == 0)).sum())
    stats["to_last"] = int((moved & (z1 == c["D"] - 1)).sum()) if c["D"] > 1 else 0
    want.setflags(write=False)
    return c, want, wsub, stats


def test_every_draw_is_inside_the_contract_and_the_same_twice():
    for seed in SEEDS:
        c, again = draw(seed), draw(seed)
        assert accepted(c), (seed, c["text"])
        assert c["text"] == again["text"]
        for k in ("disp", "vol", "sub"):
            assert (c[k] is None and again[k] is None) or c[k].tobytes() == again[k].tobytes(), (seed, k)
    assert draw(0, base=7)["text"] != draw(0)["text"]


def test_the_gpu_file_skips_nothing():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_adjust_fuzz.py")).read()
    for word in ("pytest.skip", "importorskip", "skipif", "xfail"):
        assert word not in src, word


def test_no_reference_call_is_slow():
    for seed in SEEDS:
        reference(seed)
        assert TIMES[seed] < 2.0, (seed, TIMES[seed], draw(seed)["text"])


def test_the_seeds_hold_every_regime():
    """changed and unchanged discontinuity pixels, on both axes, pixels that change in a round after the first, and changed
    pixels at both ends of the label range"""
    total = {}
    for seed in SEEDS:
        for k, v in reference(seed)[3].items():
            total[k] = total.get(k, 0) + v
    print("over the seeds:", total)
    for k in ("changed", "unchanged", "changed_h", "changed_v", "candidate_h", "candidate_v", "late", "to_first", "to_last"):
        assert total.get(k, 0) > 0, (k, total)


def test_the_seeds_hold_every_form_of_the_call():
    cs = [draw(s) for s in SEEDS]
    assert {c["form"]["in_place"] for c in cs} == {False, True} and {c["form"]["misalign"] for c in cs} == {0, 1, 255}
    assert {c["mode"] for c in cs} == {0, 1, 2} and {c["adjust"]["vertical"] for c in cs} == {0, 1}
    assert any(c["adjust"]["iterations"] == 1 for c in cs) and any(c["adjust"]["iterations"] >= 5 for c in cs)
    assert any(c["D"] > 64 for c in cs) and any(c["D"] <= 64 for c in cs)
    assert any(c["dmin"] > 0 for c in cs) and any(c["dmin"] < 0 for c in cs)
    edges = set(fs.edge_list(TILE[0], 1, 200))
    assert any(c["w"] in edges for c in cs) and any(c["w"] not in edges for c in cs) and any(c["w"] > 64 for c in cs)
    assert any(c["h"] > 4 for c in cs)
    assert any(np.isnan(c["disp"]).any() for c in cs) and any(np.isnan(c["vol"]).any() for c in cs)


def test_the_results_differ_from_the_inputs():
    changed = sum(int((reference(s)[1].view(np.uint32) != draw(s)["disp"].view(np.uint32)).any()) for s in SEEDS)
    assert changed >= 6, changed
    fits = sum(int((reference(s)[2].view(np.uint32) != draw(s)["sub"].view(np.uint32)).any()) for s in SEEDS if draw(s)["mode"])
    assert fits >= 2, fits
