"""The numpy reference of the depth-discontinuity adjustment (tests/adjust_ref.py) on its own: against a brute force written
pixel by pixel, the rules of the definition on maps built by hand, the rounds, the sub-pixel map, and the scene the feature
exists for.  Then the refusals of the C-ABI entries and of the Python layers, none of which needs a GPU: an invalid argument is
SMX_E_ARG (-1) before any device call (a device call on a machine without a GPU would be SMX_E_HIP, -2).
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import adjust_ref as ref
import cross_ref
import subpix_ref

F32 = np.float32
NAN = F32(np.nan)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def random_case(rng, h, w, dmin, size_d, specials=True, block=(3, 5)):
    """(map, volume): a blocky label map (steps of every height on both axes) with unlabelled pixels of every kind, and a volume
    of small integers (ties are common) with NaN, +-inf, -0 and denormals sprinkled in"""
    by, bx = block
    lab = rng.integers(0, size_d, (h // by + 1, w // bx + 1))
    d = (dmin + np.kron(lab, np.ones((by, bx), np.int64))[:h, :w]).astype(F32)
    m = rng.random((h, w))
    d[m < 0.08] = dmin - 100                                   # the LR marker
    d[(m >= 0.08) & (m < 0.11)] += F32(0.5)
    d[(m >= 0.11) & (m < 0.13)] = dmin + size_d                # one past the range
    d[(m >= 0.13) & (m < 0.15)] = dmin - 1
    if specials:
        d[(m >= 0.15) & (m < 0.16)] = NAN
        d[(m >= 0.16) & (m < 0.17)] = np.inf
        d[(m >= 0.17) & (m < 0.18)] = -np.inf
    if dmin <= 0 < dmin + size_d:
        d[(d == 0) & (m > 0.5)] = F32(-0.0)
    vol = rng.integers(0, 6, (size_d, h, w)).astype(F32)
    if specials:
        s = rng.random(vol.shape)
        vol[s < 0.02] = NAN
        vol[(s >= 0.02) & (s < 0.03)] = np.inf
        vol[(s >= 0.03) & (s < 0.04)] = -np.inf
        vol[(s >= 0.04) & (s < 0.06)] = F32(-0.0)
        vol[(s >= 0.06) & (s < 0.08)] = np.uint32(1).view(F32)                  # the smallest denormal
        vol[(s >= 0.08) & (s < 0.09)] = -np.uint32(0x007FFFFF).view(F32)        # the largest one, negative
    return d, vol


# ---------------------------------------------------------------------------------------------
# the reference against the brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h, w, dmin, size_d, tau_e, vertical, iterations",
                         [(9, 14, 0, 6, 2, 1, 1), (7, 11, -5, 9, 1, 1, 3), (6, 13, 3, 4, 3, 0, 2), (1, 9, -2, 5, 1, 1, 2),
                          (8, 1, 0, 5, 2, 1, 2), (5, 8, -3, 1, 1, 1, 1), (6, 9, 0, 7, 7, 1, 8)])
def test_the_reference_against_the_brute_force(h, w, dmin, size_d, tau_e, vertical, iterations):
    rng = np.random.default_rng(100 * h + w)
    d, vol = random_case(rng, h, w, dmin, size_d)
    sub = rng.normal(size=(h, w)).astype(F32)
    for mode in (subpix_ref.PARABOLA, subpix_ref.EQUIANGULAR):
        got, gsub = ref.adjust(d, vol, dmin, tau_e, vertical, iterations, mode=mode, sub=sub)
        want, wsub = ref.brute(d, vol, dmin, tau_e, vertical, iterations, mode=mode, sub=sub)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(gsub), bits(wsub))
    assert np.array_equal(bits(ref.adjust(d, vol, dmin, tau_e, vertical, iterations)), bits(want))
    lab, _ = ref.labelled(d, dmin, size_d)
    assert np.array_equal(bits(got)[~lab], bits(d)[~lab])        # an unlabelled pixel is copied bit for bit


def test_the_brute_force_cases_do_change_pixels():
    rng = np.random.default_rng(3)
    d, vol = random_case(rng, 9, 14, 0, 6)
    stats = {}
    ref.adjust(d, vol, 0, 2, 1, 2, stats=stats)
    assert stats["changed"] > 0 and stats["unchanged"] > 0 and stats["changed_v"] > 0 and stats["changed_h"] > 0


# ---------------------------------------------------------------------------------------------
# the rules, on maps built by hand: a row of three pixels, the middle one under test
# ---------------------------------------------------------------------------------------------
def row3(labels, costs_mid, size_d=8, dmin=0, **kw):
    """labels of the three pixels; costs_mid {slice: cost} of the middle pixel (every other cost 9)"""
    d = np.array([labels], F32)
    vol = np.full((size_d, 1, 3), 9, F32)
    for z, c in costs_mid.items():
        vol[z, 0, 1] = c
    return ref.adjust(d, vol, dmin, **kw)[0, 1]


def test_tau_e_at_equality():
    assert row3([1, 3, 3], {3: 5, 1: 4}, tau_e=2) == 1                  # |1 - 3| == tau_e: a candidate
    assert row3([1, 3, 3], {3: 5, 1: 4}, tau_e=3) == 3                  # one more: none
    assert row3([2, 3, 3], {3: 5, 2: 4}, tau_e=1) == 2
    assert row3([2, 3, 3], {3: 5, 2: 4}, tau_e=2) == 3


def test_the_own_label_wins_a_tie():
    assert row3([1, 4, 4], {4: 5, 1: 5}) == 4
    assert row3([1, 4, 4], {4: 5, 1: F32(4.9999995)}) == 1


def test_a_tie_between_candidates_goes_to_the_first_and_the_order_is_left_right_up_down():
    assert row3([1, 4, 7], {4: 5, 1: 3, 7: 3}) == 1                     # left before right
    assert row3([1, 4, 7], {4: 5, 1: 3, 7: 2}) == 7                     # a strictly smaller later one still wins
    d = np.array([[4, 6, 4], [0, 4, 2], [4, 7, 4]], F32)               # the middle: left 0, right 2, up 6, down 7
    for costs, want in (({0: 3, 2: 3, 6: 3, 7: 3}, 0), ({2: 3, 6: 3, 7: 3}, 2), ({6: 3, 7: 3}, 6), ({7: 3}, 7), ({}, 4),
                        ({0: 3, 7: 2}, 7)):
        vol = np.full((8, 3, 3), 9, F32)
        vol[4, 1, 1] = 5
        for z, c in costs.items():
            vol[z, 1, 1] = c
        assert ref.adjust(d, vol, 0)[1, 1] == want, costs
    # both labels equal: the first candidate's BITS are taken
    d = np.array([[F32(-0.0), 3, F32(0.0)]], F32)
    vol = np.full((8, 1, 3), 9, F32)
    vol[0, 0, 1] = 1
    assert bits(ref.adjust(d, vol, 0))[0, 1] == 0x80000000
    assert bits(ref.adjust(d[:, ::-1], vol, 0))[0, 1] == 0


def test_nan_costs():
    assert row3([1, 4, 4], {4: NAN, 1: 0}) == 4                         # a NaN own cost is never replaced
    assert row3([1, 4, 7], {4: 5, 1: NAN, 7: 6}) == 4                   # a NaN candidate never wins
    assert row3([1, 4, 7], {4: 5, 1: NAN, 7: 4}) == 7
    assert row3([1, 4, 4], {4: np.inf, 1: 3e38}) == 1
    assert row3([1, 4, 4], {4: 0.0, 1: -0.0}) == 4                      # -0 is not below +0
    assert row3([1, 4, 4], {4: 0.0, 1: -np.uint32(1).view(F32)}) == 1   # a negative denormal is


def test_minus_zero_is_the_label_zero():
    for dmin in (0, -3):
        d = np.array([[F32(-0.0), 5 + dmin, 5 + dmin]], F32) if dmin else np.array([[F32(-0.0), 5, 5]], F32)
        vol = np.full((8, 1, 3), 9, F32)
        vol[0 - dmin, 0, 1] = 1
        out = ref.adjust(d, vol, dmin)
        assert bits(out)[0, 1] == 0x80000000 and bits(out)[0, 0] == 0x80000000
    # with dmin > 0 it is out of range: not labelled, nobody's candidate
    d = np.array([[F32(-0.0), 5, 5]], F32)
    vol = np.full((8, 1, 3), 9, F32)
    vol[0] = 1
    assert np.array_equal(bits(ref.adjust(d, vol, 1)), bits(d))


@pytest.mark.parametrize("odd", [F32(-100), F32(2.5), F32(8), F32(-1), NAN, F32(np.inf), F32(-np.inf), F32(3e9), F32(-3e38)])
def test_unlabelled_values_as_the_pixel_and_as_the_neighbour(odd):
    vol = np.full((8, 1, 3), 9, F32)
    vol[:, 0, :] = np.arange(8, dtype=F32)[:, None]                     # slice 0 is everybody's cheapest
    d = np.array([[0, odd, 0]], F32)                                    # as the pixel: copied, whatever its neighbours cost
    assert np.array_equal(bits(ref.adjust(d, vol, 0, tau_e=1)), bits(d))
    d = np.array([[odd, 5, 5]], F32)                                    # as the neighbour: no candidate
    assert np.array_equal(bits(ref.adjust(d, vol, 0, tau_e=1)), bits(d))
    d = np.array([[odd, 5, 0]], F32)                                    # ... and it does not shadow the other side
    assert ref.adjust(d, vol, 0, tau_e=1)[0, 1] == 0


def test_labels_that_no_int_holds():
    """dmin may be any int: the labels at the ends of int are exact, and a float beyond them is not a label of the range"""
    vol = np.full((2, 1, 2), 9, F32)
    vol[0, 0, 1] = 1
    d = np.array([[-2147483648.0, -2147483648.0 + 256]], F32)
    lab, z = ref.labelled(d, -2 ** 31, 512)
    assert lab.all() and z.tolist() == [[0, 256]]
    lab, _ = ref.labelled(np.array([[2147483648.0]], F32), 2 ** 31 - 1, 512)
    assert lab.all()                                                    # 2^31 - (2^31 - 1) = 1
    lab, _ = ref.labelled(np.array([[2147483648.0, 3e38]], F32), 0, 512)
    assert not lab.any()


def test_vertical_0_against_1():
    d = np.array([[1, 1, 1], [4, 4, 4], [4, 4, 4]], F32)
    vol = np.full((8, 3, 3), 9, F32)
    vol[1] = 2
    assert np.array_equal(ref.adjust(d, vol, 0, vertical=0), d)
    out = ref.adjust(d, vol, 0, vertical=1)
    assert (out[1] == 1).all() and (out[2] == 4).all()
    assert (ref.adjust(d, vol, 0, vertical=1, iterations=2) == 1).all()


@pytest.mark.parametrize("iterations", range(1, 9))
def test_the_own_cost_never_rises(iterations):
    rng = np.random.default_rng(iterations)
    d, vol = random_case(rng, 12, 17, -4, 9, specials=False)
    rounds = []
    out = ref.adjust(d, vol, -4, 1, 1, iterations, rounds=rounds)
    assert len(rounds) == iterations and np.array_equal(bits(rounds[-1]), bits(out))
    cost = ref.own_cost(d, vol, -4)
    moved = 0
    for m in rounds:
        nxt = ref.own_cost(m, vol, -4)
        assert np.array_equal(np.isnan(nxt), np.isnan(cost))            # labelled stays labelled, unlabelled unlabelled
        assert (nxt[~np.isnan(nxt)] <= cost[~np.isnan(cost)]).all()
        moved += int((nxt < cost).sum())
        cost = nxt
    assert moved > 0
    # Jacobi: a round reads the snapshot only, so it equals one call on the map of the round before
    again = d
    for k in range(iterations):
        again = ref.adjust(again, vol, -4, 1, 1, 1)
        assert np.array_equal(bits(again), bits(rounds[k]))


def test_an_edge_moves_one_pixel_a_round():
    d = np.array([[1] * 3 + [5] * 7], F32)
    vol = np.full((8, 1, 10), 9, F32)
    vol[1] = 2                                                          # the whole row is label 1 by its costs
    for k in range(1, 8):
        out = ref.adjust(d, vol, 0, iterations=k)
        assert (out[0, :3 + k] == 1).all() and (out[0, 3 + k:] == 5).all()


@pytest.mark.parametrize("mode", [subpix_ref.PARABOLA, subpix_ref.EQUIANGULAR])
def test_the_sub_pixel_map(mode):
    size_d = 6
    # the middle pixel changes to slice 0, to slice size_d - 1 and to one inside; its neighbours do not change
    for znew in (0, size_d - 1, 2):
        zold = 3 if znew != 3 and abs(znew - 3) >= 2 else 0
        d = np.array([[znew, zold, zold]], F32)
        vol = np.full((size_d, 1, 3), 9, F32)
        vol[:, 0, 1] = [7, 6, 4, 8, 5, 3]
        vol[znew, 0, 1] = 1
        sub = np.array([[0.25, 0.5, 0.75]], F32)
        out, s = ref.adjust(d, vol, 0, mode=mode, sub=sub)
        assert out[0, 1] == znew
        assert s[0, 0] == F32(0.25) and s[0, 2] == F32(0.75)            # untouched where the label stayed
        lo = vol[znew - 1, 0, 1] if znew > 0 else NAN
        hi = vol[znew + 1, 0, 1] if znew + 1 < size_d else NAN
        want = F32(znew) + subpix_ref.delta(mode, F32(1), lo, hi)
        assert bits(s)[0, 1] == bits(want)
        if znew in (0, size_d - 1):
            assert s[0, 1] == znew                                      # a neighbour outside the range: delta 0
        else:
            assert s[0, 1] != znew
            assert s[0, 1] == F32(znew) + F32(smx.subpixel_delta("parabola" if mode == subpix_ref.PARABOLA else "equiangular",
                                                                 1.0, float(lo), float(hi)))


# ---------------------------------------------------------------------------------------------
# the reason for the feature
# ---------------------------------------------------------------------------------------------
DMIN, SIZE_D = -7, 8
BLOCK = (slice(8, 16), slice(24, 32))
CROSS = dict(l1=17, l2=8, tau1=20, tau2=6)


def step_case(orc):
    """cross_ref.step_scene's two surfaces as a left view's labels (d = z - 7: the left surface -5, the nearer one, the right
    surface -2); a block of 8 x 8 of the left, foreground surface, flush against the step, rejected as the LR check rejects
    (the marker dmin - 100); the oracle's scan-line fill over it; and the cross-based aggregation of the scene's noisy costs on
    its colour guide, whose regions end at the colour edge: a volume that favours each surface's own label.
    -> (filled map, volume, truth, rejected map)"""
    g, cost, z = cross_ref.step_scene(seed=1)
    truth = (z + DMIN).astype(F32)
    assert (truth[BLOCK] == -5).all() and (truth[:, 32] == -2).all()
    d = truth.copy()
    d[BLOCK] = DMIN - 100
    filled = orc.fill_occlusion(d, float(DMIN))
    vol = cross_ref.aggregate(g, cost, **CROSS)
    assert np.array_equal(cross_ref.winners(vol), z)                    # the costs favour each surface's own label
    return filled, vol, truth, d


STEP_COUNTS = (64, 42, 0)       # wrong pixels of the block: after the fill alone, after one round, after eight


def test_the_block_beside_the_step(orc):
    """The fill paints the rejected block with the background's label (the larger of a row's two neighbours), so the edge of
    the map lies 8 pixels from the edge of the object.  A round moves it back by one pixel from every side on which the block
    touches its own surface; as many rounds as the block is wide bring all of it back."""
    filled, vol, truth, _ = step_case(orc)
    wrong = [int((filled[BLOCK] != truth[BLOCK]).sum())]
    for it in (1, 8):
        out = ref.adjust(filled, vol, DMIN, tau_e=2, vertical=1, iterations=it)
        wrong.append(int((out[BLOCK] != truth[BLOCK]).sum()))
        outside = np.ones(truth.shape, bool)
        outside[BLOCK] = False
        assert np.array_equal(out[outside], truth[outside])             # and nothing that was right is broken
    print(f"step scene: wrong pixels of the block after the fill alone {wrong[0]}, after one round {wrong[1]}, "
          f"after eight {wrong[2]}")
    assert wrong[0] == 64 and wrong[2] == 0 and wrong[0] > wrong[1] > wrong[2]
    assert tuple(wrong) == STEP_COUNTS
    # the rows alone need the same eight rounds: the edge comes from one side only
    rows = [int((ref.adjust(filled, vol, DMIN, vertical=0, iterations=it)[BLOCK] != truth[BLOCK]).sum()) for it in (1, 7, 8)]
    assert rows == [56, 8, 0]


# ---------------------------------------------------------------------------------------------
# refusals: no GPU needed
# ---------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(tau_e=0), dict(tau_e=-1), dict(tau_e=513), dict(vertical=2), dict(vertical=-1), dict(iterations=0),
              dict(iterations=9), dict(iterations=-1), dict(tau_e=0, iterations=20)]


def _params(**kw):
    p = smx.default_adjust_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_and_workspace_size():
    L = smx.lib()
    p = smx.default_adjust_params()
    assert (p.tau_e, p.vertical, p.iterations) == (2, 1, 1)
    assert ref.params_ok(**ref.DEFAULTS) and ref.DEFAULTS == {k: getattr(p, k) for k in ref.DEFAULTS}
    assert L.smx_adjust_workspace_bytes(7, 5) == 255 + 8 * 35
    assert L.smx_adjust_workspace_bytes(1, 70000) > 0
    for bad in ((0, 5), (5, 0), (-1, 5), (65536, 32768)):
        assert L.smx_adjust_workspace_bytes(*bad) == 0, bad
    tw, th = C.c_int(0), C.c_int(0)
    assert L.smx_adjust_geometry(C.byref(tw), C.byref(th)) == 0 and tw.value >= 1 and th.value >= 1
    assert L.smx_adjust_geometry(None, C.byref(th)) == -1
    for ok in (dict(tau_e=1), dict(tau_e=512), dict(iterations=8), dict(vertical=0)):
        assert ref.params_ok(**{**ref.DEFAULTS, **ok})


def test_every_entry_refuses_invalid_arguments_before_any_device_call():
    L = smx.lib()
    x = C.c_void_p(4096)            # never dereferenced: every call below fails its checks
    wsb = L.smx_adjust_workspace_bytes(7, 5)

    def dev(p, d=x, a=x, out=x, w=7, h=5, D=4, mode=0, sub=None, ws=x, wsb=wsb):
        return L.smx_dev_discontinuity_adjust(p, d, a, out, w, h, 0, D, mode, sub, ws, wsb, None)

    def host(p, d=x, a=x, out=x, w=7, h=5, D=4, mode=0, sub=None):
        return L.smx_discontinuity_adjust(p, d, a, out, w, h, 0, D, mode, sub)

    for bad in BAD_PARAMS:
        assert not ref.params_ok(**{**ref.DEFAULTS, **bad}), bad
        p = C.byref(_params(**bad))
        for entry in (dev, host):
            assert entry(p) == -1, (entry.__name__, bad)
            assert b"tau_e" in L.smx_last_error()
        assert L.smx_ctx_set_adjust(None, p) == -1
    ok = C.byref(_params())
    for entry in (dev, host):
        assert entry(None) == -1
        for kw in (dict(w=0), dict(h=0), dict(w=-3), dict(w=65536, h=32768), dict(D=0), dict(D=513), dict(D=-1), dict(d=None),
                   dict(a=None), dict(out=None), dict(mode=3), dict(mode=-1), dict(sub=x, mode=0), dict(sub=x, mode=3)):
            assert entry(ok, **kw) == -1, (entry.__name__, kw)
    assert not any(ref.shape_ok(*s) for s in ((0, 5, 4), (7, 0, 4), (65536, 32768, 4), (7, 5, 0), (7, 5, 513))) and ref.shape_ok(7, 5, 512)
    # the workspace: one byte short, or missing, is SMX_E_WS before anything is launched
    assert dev(ok, wsb=wsb - 1) == -3 and b"workspace" in L.smx_last_error()
    assert dev(ok, ws=None) == -3
    assert L.smx_ctx_set_adjust(None, ok) == -1 and L.smx_ctx_set_adjust(None, None) == -1


def test_the_python_layers_refuse():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    d = np.zeros((5, 7), F32)
    a = np.zeros((4, 5, 7), F32)
    for bad in (dict(disparity=np.zeros((2, 5, 7), F32)), dict(agg=np.zeros((5, 7), F32)), dict(agg=np.zeros((4, 5, 6), F32)),
                dict(params=smx.default_vote_params()), dict(subpixel="cubic", sub=d), dict(subpixel="parabola"), dict(sub=d),
                dict(subpixel="parabola", sub=np.zeros((5, 6), F32))):
        kw = dict(disparity=d, agg=a, dmin=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            smx.discontinuity_adjust(**kw)
    for bad in (dict(params=_params(tau_e=0)), dict(params=_params(iterations=9)), dict(agg=np.zeros((513, 5, 7), F32))):
        kw = dict(disparity=d, agg=a, dmin=0)
        kw.update(bad)
        with pytest.raises(smx.SmxError) as e:
            smx.discontinuity_adjust(**kw)
        assert e.value.code == -1
    for kw in (dict(adjust="yes"), dict(adjust=smx.default_vote_params()), dict(adjust=_params(tau_e=0)),
               dict(adjust=True, s_begin=1), dict(adjust=True, s_end=7), dict(adjust=True, max_ws_bytes=1000)):
        with pytest.raises(ValueError):
            PairPipeline(64, 24, 8, device="cpu", **kw)
    with pytest.raises(ValueError):
        PairPipeline(64, 24, 513, device="cpu", adjust=True)
    for kw in (dict(adjust=True), dict(adjust=smx.default_adjust_params())):
        with pytest.raises(ValueError, match="adjustment"):
            ShardedPair(64, 24, 8, **kw)
    assert isinstance(smx.default_adjust_params(), _lib.AdjustParams) and smx.AdjustParams is _lib.AdjustParams
