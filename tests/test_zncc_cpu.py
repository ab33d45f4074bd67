"""The ZNCC window matching cost without a GPU: the properties of the definition on tests/zncc_ref.py, the host-only entries of
the library, and what the cost is for -- the scene of DESIGN.md 4.3u, a pair whose right image carries a gain and an offset
that change across the image, run through the oracle's guided filter, the LR check and the fill.

Wrong labels are counted among the 7200 kept pixels on the winner-take-all left map (`dmapl`, "wta" below: what the cost and
the aggregation decide) and on the final filled map ("filled").  The counts are deterministic and asserted as measured.
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import census_ref
import mi_ref
import zncc_ref as ref

F32 = np.float32
WINDOWS = [(1, 1), (1, 4), (4, 1), (4, 4), (3, 3)]


# ---------------------------------------------------------------------------------------------
# properties of the definition
# ---------------------------------------------------------------------------------------------
def _texture(seed, h=24, w=60, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w)).astype(np.uint8)


@pytest.mark.parametrize("a,b", [(1, 0), (2, 19), (0.5, 31), (1.5, -20)])
@pytest.mark.parametrize("rx,ry", WINDOWS)
def test_an_affine_change_costs_nothing_at_the_true_label(rx, ry, a, b):
    """B = a A + b shifted by 5 (A even, so that a A + b is an integer: nothing rounded, nothing clipped): cost 0 at label -5
    wherever neither window is flat.  num = a Va and Vb = a^2 Va, so s is 1 up to the last bits of three roundings."""
    A = (2 * _texture(1, lo=10, hi=60)).astype(np.uint8)
    Bw = a * A.astype(np.float64) + b
    assert np.array_equal(Bw, np.rint(Bw)) and Bw.min() >= 0 and Bw.max() <= 255
    B = np.roll(Bw.astype(np.uint8), -5, axis=1)              # B[x] = Bw[x + 5]: A[x] corresponds to B[x - 5]
    cost = ref.zncc_cost(A, B, 8, -7, rx, ry)
    inner = slice(5 + rx, A.shape[1] - rx)                    # windows that meet neither the wrap of the roll nor the clamp
    assert np.all(ref.moments(A, rx, ry)[1][:, inner] > 0)
    assert np.all(cost[2][:, inner] == 0.0), (a, b)
    assert cost[[0, 1, 3, 4]][:, :, inner].mean() > 64.0       # and the other labels are far from it (128 where uncorrelated)


def test_a_flat_window_costs_128_and_a_partner_outside_255():
    A = _texture(2)
    flat = np.full_like(A, 99)
    for own, other in ((A, flat), (flat, A), (flat, flat)):
        c = ref.zncc_cost(own, other, 5, -2)
        for z in range(5):
            d = z - 2
            x0, x1 = max(0, -d), min(A.shape[1], A.shape[1] - d)
            assert np.all(c[z][:, x0:x1] == 128.0)
            assert np.all(c[z][:, :x0] == 255.0) and np.all(c[z][:, x1:] == 255.0)
    # a flat patch inside a texture: 128 exactly where one of the two windows lies inside the patch
    B = A.copy()
    B[4:20, 10:40] = 7
    c = ref.zncc_cost(A, B, 1, 0)[0]
    assert np.all(c[7:17, 13:37] == 128.0) and not np.any(c[:4] == 128.0)
    # labels whose partners all lie outside
    assert np.all(ref.zncc_cost(A, A, 3, A.shape[1]) == 255.0) and np.all(ref.zncc_cost(A, A, 3, -A.shape[1] - 2) == 255.0)


@pytest.mark.parametrize("rx,ry", WINDOWS)
def test_an_inverted_partner_costs_255(rx, ry):
    A = _texture(3)
    c = ref.zncc_cost(A, 255 - A, 1, 0, rx, ry)[0]
    assert np.all(ref.moments(A, rx, ry)[1] > 0)
    assert np.all(c == 255.0)
    assert np.all(ref.zncc_cost(A, A, 1, 0, rx, ry)[0] == 0.0)


def test_the_extreme_stays_inside_32_bits():
    """All 255 against a 0 / 255 checkerboard at 9 x 9, and the checkerboard against itself and against its inverse: the largest
    N P, S_A S_B and V the definition can meet, and |num| at its largest."""
    h, w = 12, 14
    yy, xx = np.mgrid[0:h, 0:w]
    white = np.full((h, w), 255, np.uint8)
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    stats = {}
    c = ref.zncc_cost(white, board, 3, -1, 4, 4, stats=stats)
    inside = c != 255.0
    assert np.all(c[inside] == 128.0)                          # the white window is flat
    ref.zncc_cost(white, white, 1, 0, 4, 4, stats=stats)
    assert stats["NP"] == 81 * 81 * 65025 and stats["SS"] == (81 * 255) ** 2 and stats["num"] == 0
    s2 = {}
    same = ref.zncc_cost(board, board, 1, 0, 4, 4, stats=s2)[0]
    inv = ref.zncc_cost(board, 255 - board, 1, 0, 4, 4, stats=s2)[0]
    assert np.all(same == 0.0) and np.all(inv == 255.0)
    assert s2["V"] == 81 * 41 * 65025 - (41 * 255) ** 2 == 40 * 41 * 65025    # the largest variance of 81 values in 0 .. 255
    assert s2["num"] == s2["V"]                                 # |num| <= sqrt(Va Vb) (Cauchy-Schwarz), met with equality
    for v in list(stats.values()) + list(s2.values()):
        assert 0 <= v < 2 ** 31
    assert 81 * 81 * 65025 < 2 ** 31


def test_moment_words_pack_s_and_v():
    A = _texture(4, 5, 9)
    S, V = ref.moments(A, 2, 1)
    words = ref.moment_words(A, 2, 1)
    assert np.array_equal(words & np.uint64(0xFFFFFFFF), S.astype(np.uint64))
    assert np.array_equal(words >> np.uint64(32), V.astype(np.uint64))
    # the window of (0, 0), clamped: rows 0, 0, 1 and columns 0, 0, 0, 1, 2
    assert S[0, 0] == 2 * (3 * int(A[0, 0]) + int(A[0, 1]) + int(A[0, 2])) + 3 * int(A[1, 0]) + int(A[1, 1]) + int(A[1, 2])


def test_sub_ranges_are_slices_of_the_volume():
    A, B = _texture(5), _texture(6)
    full = ref.zncc_cost(A, B, 9, -4, 2, 3)
    assert np.array_equal(ref.zncc_cost(A, B, 9, -4, 2, 3, 2, 7), full[2:7])
    assert set(np.unique(full)) <= set(np.arange(256, dtype=F32))
    assert ref.zncc_cost(A, B, 9, -4, 2, 3, 4, 4).shape == (0,) + A.shape


# ---------------------------------------------------------------------------------------------
# the host-only entries of the library (the built library, no device)
# ---------------------------------------------------------------------------------------------
def _zp(rx, ry):
    p = _lib.ZnccParams()
    p.rx, p.ry = rx, ry
    return p


def test_window_and_defaults():
    L = smx.lib()
    p = smx.default_zncc_params()
    assert (p.rx, p.ry) == ref.DEFAULTS == (3, 3)
    assert L.smx_zncc_window(C.byref(p)) == 49
    for rx in range(1, 5):
        for ry in range(1, 5):
            assert L.smx_zncc_window(C.byref(_zp(rx, ry))) == ref.window(rx, ry)
    for rx, ry in ((0, 3), (3, 0), (5, 3), (3, 5), (-1, 1), (1 << 20, 1)):
        assert L.smx_zncc_window(C.byref(_zp(rx, ry))) == -1
    assert L.smx_zncc_window(None) == -1
    cols, rows = C.c_int(), C.c_int()
    assert L.smx_zncc_geometry(C.byref(cols), C.byref(rows)) == 0 and cols.value > 8 and rows.value >= 1
    assert L.smx_zncc_geometry(None, C.byref(rows)) == -1


def test_argument_checks_come_before_the_device():
    L = smx.lib()
    img = np.zeros((4, 5), np.uint8)
    cost = np.zeros((2, 4, 5), F32)
    P = lambda a: a.ctypes.data
    good = C.byref(_zp(3, 3))
    for args in ((C.byref(_zp(5, 1)), P(img), P(img), P(cost), 5, 4, 2, 0), (None, P(img), P(img), P(cost), 5, 4, 2, 0),
                 (good, None, P(img), P(cost), 5, 4, 2, 0), (good, P(img), None, P(cost), 5, 4, 2, 0),
                 (good, P(img), P(img), None, 5, 4, 2, 0), (good, P(img), P(img), P(cost), 0, 4, 2, 0),
                 (good, P(img), P(img), P(cost), 5, 0, 2, 0), (good, P(img), P(img), P(cost), 5, 4, 0, 0)):
        assert L.smx_zncc_cost(*args) == -1
    assert not cost.any()
    assert "1 <= rx <= 4" in (L.smx_zncc_cost(C.byref(_zp(5, 1)), P(img), P(img), P(cost), 5, 4, 2, 0), L.smx_last_error().decode())[1]
    assert L.smx_dev_zncc_moments(C.byref(_zp(0, 1)), P(img), P(cost), 5, 4, 1, None) == -1
    assert L.smx_dev_zncc_cost_pair(good, P(cost), P(img), P(img), None, None, 5, 4, 0, 0, 0, 2, None) == -1
    with pytest.raises(ValueError):
        smx.zncc_cost(img, np.zeros((4, 6), np.uint8), 2, 0)
    with pytest.raises(smx.SmxError):
        smx.zncc_cost(img, img, 0, 0)


def test_the_context_setter_needs_a_context_and_the_cost_setter_refuses_the_mode():
    L = smx.lib()
    assert L.smx_ctx_set_zncc(None, C.byref(_zp(3, 3))) == -1 and L.smx_ctx_set_zncc(None, None) == -1
    assert L.smx_ctx_set_cost(None, 3, None) == -1
    assert _lib.COST_MODES == {"reference": 0, "census": 1}


# ---------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------
D, DMINL, DMINR = ref.SCENE_D, ref.SCENE_DMIN, 0
KEPT = 7200
_COUNTS = {}


def counts(orc, seed):
    """(wta, filled) wrong-label counts per cost: the reference's, census, MI at its defaults (three tables from the random
    start) and ZNCC at its defaults."""
    if seed not in _COUNTS:
        Il, Ir, truth, kept = ref.scene(seed)
        assert int(kept.sum()) == KEPT

        def solve(cl, cr):
            _, ml, _, _ = orc.guided_filter(Il, cl, DMINL)
            _, mr, _, _ = orc.guided_filter(Ir, cr, DMINR)
            occ = orc.detect_occlusion(ml, mr, DMINL - 100)
            return dict(dmapl=ml, dmapr=mr, occlusion=occ, filled=orc.fill_occlusion(occ, float(DMINL)))

        def both(r):
            return ref.wrong(r["dmapl"], truth, kept), ref.wrong(r["filled"], truth, kept)

        def refc():
            return orc.cost_volume(Il, Ir, D, DMINL), orc.cost_volume(Ir, Il, D, DMINR)

        _COUNTS[seed] = {
            "reference": both(solve(*refc())),
            "census": both(solve(census_ref.census_cost(Il, Ir, D, DMINL), census_ref.census_cost(Ir, Il, D, DMINR))),
            "mi": both(mi_ref.pair_loop(Il, Ir, D, DMINL, DMINR, solve, 3, mi_ref.INIT_RANDOM, 0, refc)[-1]),
            "zncc": both(solve(ref.zncc_cost(Il, Ir, D, DMINL), ref.zncc_cost(Ir, Il, D, DMINR)))}
    return _COUNTS[seed]


# (wta, filled) as measured with the oracle's guided filter (radius 9, the defaults); README.md and DESIGN.md 4.3u hold the same
MEASURED = {
    0: {"reference": (563, 72), "census": (265, 90), "mi": (4324, 3951), "zncc": (0, 20)},
    1: {"reference": (587, 124), "census": (248, 41), "mi": (3057, 1286), "zncc": (6, 0)},
}


def test_the_scene_is_what_it_says():
    Il, Ir, truth, kept = ref.scene(0)
    assert Il.shape == Ir.shape == (ref.SCENE_H, ref.SCENE_W) and Il.dtype == Ir.dtype == np.uint8
    x = np.arange(ref.SCENE_W)
    for y in (3, 20):                                           # a row of the texture, a row of the band
        for a, b in ref.SCENE_KEPT:
            xs = x[a:b]
            d = truth[y, xs].astype(np.int64)
            t = (xs + d) / (ref.SCENE_W - 1.0)
            want = np.rint(Il[y, xs] * (0.6 + 0.8 * t) + 80.0 * t)
            assert np.array_equal(Ir[y, xs + d], want.astype(np.uint8))      # right = gain * left + offset, nothing clipped
    assert 0 < Ir.min() and Ir.max() < 255
    # the band, away from its first and last rows: census cannot tell the true label from the one a period away (its two
    # lowest mean costs, half a bit apart at the most), ZNCC can
    P = ref.SCENE_PERIOD
    rows, cols = slice(ref.SCENE_BAND[0] + 4, ref.SCENE_BAND[1] - 4), slice(24, 56)
    cen = census_ref.census_cost(Il, Ir, D, DMINL)[:, rows, cols].mean(axis=(1, 2))
    z = ref.zncc_cost(Il, Ir, D, DMINL)[:, rows, cols].mean(axis=(1, 2))
    true, away = -4 - DMINL, -4 - P - DMINL
    assert set(np.argsort(cen)[:2]) == {true, away} and abs(cen[true] - cen[away]) < 0.5
    assert np.argmin(z) == true and z[away] - z[true] > 2.0


@pytest.mark.parametrize("seed", [0, 1])
def test_scene_counts_are_the_measured_ones(orc, seed):
    row = counts(orc, seed)
    print(f"\nseed {seed}: {row}")
    assert row == MEASURED[seed]


@pytest.mark.parametrize("seed", [0, 1])
def test_zncc_finds_the_labels_where_the_other_costs_do_not(orc, seed):
    """The condition of the feature, on the winner-take-all left map: ZNCC is wrong on at most 1 % of the kept pixels, the
    reference's cost, census and mutual information each on at least ten times as many.

    Why each of them fails here.  Mutual information learns one table for the image, and across this image the right view grows
    brighter where the left one grows darker: the table holds that falling relation, and inside a window, where the relation
    rises, it prefers the wrong partner (4324 and 3057 wrong).  Census cannot tell the labels one period apart in the band
    (265, 248, all of them in the band's rows), and the reference's cost, whose two truncated terms saturate under the gain,
    loses the band too (563, 587).  ZNCC is wrong on 0 and 6 pixels.  On the filled map the LR check and the fill blur the
    picture: they repair most of census's and the reference's band and cost ZNCC 20 pixels that the fill takes from a neighbour
    (seed 0); the counts are in MEASURED, the condition is on the map the costs decide."""
    row = counts(orc, seed)
    assert row["zncc"][0] <= KEPT // 100
    for other in ("reference", "census", "mi"):
        assert row[other][0] >= 10 * max(row["zncc"][0], 1), other
