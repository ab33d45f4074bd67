"""The numpy reference of the information permeability filter (tests/perm_ref.py; the definition above smx_perm_params in
include/smx.h) on the CPU: the properties the definition states, and what the filter buys on two synthetic scenes behind the
oracle's guided filter.

The scenes (192 x 48, 16 labels from -15):
  band   the scene of tests/test_cscale_cpu.py, restated here: random texture with a constant band of 60 columns (left columns
         60 .. 119), true label -6.  The guided filter alone leaves most of the band wrong; cross-scale aggregation brings it to
         within one label; the permeability pass at sigma 32 over the guided filter's volume brings every pixel of it onto the
         label.  On the RAW cost volume (the paper's own form) the band is exact too at sigma 32, while the textured columns
         keep a few errors: there every permeability is near 0 and a pixel keeps its own raw cost -- the documented limit, printed
         and not asserted.
  step   background gray 90 +- 6 with label -2, a foreground block of gray 170 +- 6 at left columns 80 .. 139 with label -8,
         noise sigma 1: the left columns 74 .. 79 are occluded.  The edge stays where it is.
"""
import numpy as np
import pytest

import perm_ref as ref

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# the definition's properties
# ---------------------------------------------------------------------------------------------
def test_table():
    for sigma in (32.0, 16.0, 0.001, 1e6):
        t = ref.table(sigma)
        assert t.dtype == F32 and t.shape == (256,) and t[0] == 1.0 and (np.diff(t) <= 0).all()
    assert (ref.table(0.001)[1:] == 0).all()
    t = ref.table(0.011)                # exp(-1 / 0.011) = 3.3e-40: below the smallest normal float
    assert 0 < t[1] < np.finfo(F32).tiny and t[2] == 0
    t = ref.table(0.012)                # exp(-1 / 0.012) = 6.5e-37, exp(-2 / 0.012) underflows
    assert 0 < t[1] < 1e-36 and t[2] == 0


def _alternating_guide(h, w):
    """every pair of neighbours differs"""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) % 2) * 200 + 20).astype(np.uint8)


def test_zero_permeability_returns_the_volume_bit_for_bit():
    rng = np.random.default_rng(1)
    h, w = 9, 13
    vol = (rng.standard_normal((4, h, w)) * 1e3).astype(F32)
    vol[0, 0, 0] = np.finfo(F32).max / 2 * F32(0.99)
    vol[1, 2, 3] = -np.finfo(F32).max / 2 * F32(0.99)
    vol[2, 4, 4] = -0.0
    vol[3, 1, 1] = np.finfo(F32).tiny / 4
    out = ref.filter_volume(vol, _alternating_guide(h, w), 0.001)
    # ((c + c) - c is c for every finite |c| < FLT_MAX / 2; -0 comes back as +0 + -0 ... = 0 with the sign of the sums)
    same = bits(out) == bits(vol)
    assert same[vol != 0].all() and (out[vol == 0] == 0).all()


def test_constant_guide_sums_the_slice():
    rng = np.random.default_rng(2)
    h, w = 6, 11
    vol = rng.integers(-8, 9, (3, h, w)).astype(F32)        # (small integers: every order of summation is exact)
    for guide in (np.full((h, w), 77, np.uint8), np.full((h, w, 3), 5, np.uint8), np.full((h, w, 4), 250, np.uint8)):
        out = ref.filter_volume(vol, guide, 32.0)
        assert (out == vol.sum(axis=(1, 2), dtype=np.float64)[:, None, None]).all()
    # in the order the recurrences define: against the loops on a volume whose sums do round
    vol = rng.standard_normal((2, h, w)).astype(F32)
    g = np.full((h, w), 3, np.uint8)
    assert np.array_equal(bits(ref.filter_volume(vol, g, 32.0)), bits(ref.filter_volume_loops(vol, g, 32.0)))


def test_alpha_is_ignored_and_colour_takes_the_maximum():
    rng = np.random.default_rng(3)
    g = rng.integers(0, 256, (5, 7, 4)).astype(np.uint8)
    g2 = g.copy()
    g2[:, :, 3] = rng.integers(0, 256, (5, 7))
    a, b = ref.weights(g, 20.0), ref.weights(g2, 20.0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = ref.weights(g[:, :, :3], 20.0)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    t = ref.table(20.0)
    d = np.abs(g[2, 3, :3].astype(int) - g[2, 2, :3].astype(int)).max()
    assert a[0][2, 3] == t[d]
    one = ref.weights(g[:, :, :1], 20.0)
    assert np.array_equal(one[0], ref.weights(g[:, :, 0], 20.0)[0])


@pytest.mark.parametrize("sigma", [32.0, 0.012, 0.011, 3.0])
@pytest.mark.parametrize("ch", [1, 3])
def test_loops_equal_the_vectorised_reference(sigma, ch):
    """7 x 5 x 3, with a NaN, an infinity and a -0; sigma 0.012 and 0.011: products with tiny and subnormal weights"""
    rng = np.random.default_rng(int(sigma * 1000) + ch)
    w, h, D = 7, 5, 3
    vol = rng.standard_normal((D, h, w)).astype(F32)
    vol[0, 1, 2] = np.nan
    vol[1, 3, 0] = np.inf
    vol[2, 0, 6] = -0.0
    g = (rng.integers(0, 3, (h, w, ch)) + 100).astype(np.uint8)         # (neighbours differ by 0, 1 or 2)
    a = ref.filter_volume(vol, g if ch > 1 else g[:, :, 0], sigma)
    b = ref.filter_volume_loops(vol, g if ch > 1 else g[:, :, 0], sigma)
    nan = np.isnan(a) & np.isnan(b)
    assert ((bits(a) == bits(b)) | nan).all() and nan.sum() == np.isnan(a).sum()


def test_single_row_column_and_pixel():
    rng = np.random.default_rng(4)
    for h, w in ((1, 1), (1, 6), (6, 1), (2, 2)):
        vol = rng.standard_normal((2, h, w)).astype(F32)
        g = rng.integers(0, 256, (h, w)).astype(np.uint8)
        assert np.array_equal(bits(ref.filter_volume(vol, g, 9.0)), bits(ref.filter_volume_loops(vol, g, 9.0)))
    one = rng.standard_normal((3, 1, 1)).astype(F32)
    assert np.array_equal(bits(ref.filter_volume(one, np.zeros((1, 1), np.uint8))), bits(one))


def test_winners_follow_the_packed_key_rule():
    q = np.array([[[1.0, np.nan]], [[0.5, np.nan]], [[0.5, np.nan]], [[2.0, np.nan]]], F32)
    z, c0 = ref.winners(q)
    assert z.tolist() == [[2, -1]] and c0[0, 0] == 0.5
    assert ref.pack_keys(z, c0)[0, 1] == np.iinfo(np.int64).max


# ---------------------------------------------------------------------------------------------
# what the method buys
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL, DMINR = 192, 48, 16, -15, 0


def band_scene(seed, d, B):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, 224)).astype(np.float64)
    base[:, 76:76 + B] = 128
    L = base[:, 16:208] + rng.normal(0, 1, (H, W))
    R = base[:, 16 + d:208 + d] + rng.normal(0, 1, (H, W))
    return tuple(np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in (L, R))


def step_scene(seed):
    rng = np.random.default_rng(seed)
    bg = 90.0 + rng.integers(-6, 7, (H, W + 16))
    fg = 170.0 + rng.integers(-6, 7, (H, 60))
    L, R = bg[:, :W].copy(), bg[:, 2:W + 2].copy()          # background: label -2
    L[:, 80:140] = fg
    R[:, 72:132] = fg                                       # foreground: label -8
    L, R = L + rng.normal(0, 1, (H, W)), R + rng.normal(0, 1, (H, W))
    truth = np.full((H, W), -2.0)
    truth[:, 80:140] = -8.0
    return tuple(np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in (L, R)) + (truth,)


def _labels(vol):
    return ref.label_map(ref.winners(vol)[0], DMINL)


def _off(m, d, c0, c1, by):
    return int((np.abs(m[:, c0:c1] + d) > by).sum())


@pytest.fixture(scope="module", params=[0, 1])
def band(request):
    import oracle
    d, B = 6, 60
    L, R = band_scene(request.param, d, B)
    r = oracle.stereo_pair(L, R, D, dminl=DMINL, dminr=DMINR, want_cost=True, want_agg=True)
    return request.param, d, B, L, r["costl"], r["aggl"]


def test_permeability_behind_the_guided_filter_repairs_the_band_exactly(band):
    seed, d, B, L, cost, agg = band
    fine = _labels(agg)
    perm = _labels(ref.filter_volume(agg, L, 32.0))
    print(f"seed {seed}: band off by more than 1: guided filter {_off(fine, d, 60, 60 + B, 1)}, permeability",
          _off(perm, d, 60, 60 + B, 1), "| wrong exact label in the band: guided filter", _off(fine, d, 60, 60 + B, 0),
          "permeability", _off(perm, d, 60, 60 + B, 0), "| errors in columns 20..59:", _off(perm, d, 20, 60, 0))
    assert _off(perm, d, 60, 60 + B, 0) == 0
    assert _off(perm, d, 20, 60, 0) == 0
    assert _off(fine, d, 60, 60 + B, 1) >= 500


def test_permeability_on_the_raw_cost_volume(band):
    """the paper's own form: the band is exact at sigma 32; the errors in the textured columns are the documented limit (7 / 15
    for seeds 0 / 1 in the draft the issue reports; printed here, not asserted), and so are the figures at sigma 16 and 24"""
    seed, d, B, L, cost, agg = band
    for sigma in (16.0, 24.0, 32.0):
        m = _labels(ref.filter_volume(cost, L, sigma))
        print(f"seed {seed}: raw cost volume, sigma {sigma}: wrong exact label in the band {_off(m, d, 60, 60 + B, 0)}, "
              f"errors in columns 20..59 {_off(m, d, 20, 60, 0)}")
    assert _off(m, d, 60, 60 + B, 0) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_depth_step_stays_where_it_is(seed):
    import oracle
    L, R, truth = step_scene(seed)
    agg = oracle.stereo_pair(L, R, D, dminl=DMINL, dminr=DMINR, want_agg=True)["aggl"]
    keep = np.ones(W, bool)
    keep[:20] = False
    keep[74:80] = False             # (occluded in the right view)
    for sigma in (16.0, 32.0, 64.0):
        m = _labels(ref.filter_volume(agg, L, sigma))
        wrong = int((m != truth)[:, keep].sum())
        print(f"seed {seed}: step scene, sigma {sigma}: wrong outside the occluded columns {wrong}, inside",
              int((m != truth)[:, 74:80].sum()))
        if sigma == 32.0:
            at32 = wrong
    assert at32 == 0
