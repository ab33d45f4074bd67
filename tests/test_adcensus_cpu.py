"""The AD-Census matching cost without a GPU: the host tables of the C-ABI against numpy and their hard properties, the
argument checks (made before the device is touched), the refusals of the Python layer, and the numpy reference of
tests/adcensus_ref.py on the scene the cost exists for and on a hand-worked image."""
import ctypes as C
import math

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import adcensus_ref as ref
import census_ref

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _params(lc=30.0, la=10.0, scale=127.5, colour=0, rx=4, ry=3, th=62):
    p = _lib.AdCensusParams()
    p.census.rx, p.census.ry, p.census.th = rx, ry, th
    p.lambda_census, p.lambda_ad, p.scale, p.colour = lc, la, scale, colour
    return p


def test_defaults(lib):
    p = smx.default_adcensus_params()
    d = ref.DEFAULTS
    assert (p.census.rx, p.census.ry, p.census.th) == (d["rx"], d["ry"], d["th"]) == census_ref.DEFAULTS
    assert (p.lambda_census, p.lambda_ad, p.scale, p.colour) == (30.0, 10.0, 127.5, 0)
    assert _lib.ADCENSUS_TABLE_FLOATS == ref.TABLE_FLOATS == 64 + 766
    lib.smx_default_adcensus_params(None)             # a NULL pointer is ignored


def _ulps(a, b):
    """Distance in units of the last place between two arrays of non-negative finite float32."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("lc,la,scale,colour", [(30.0, 10.0, 127.5, 0), (1e6, 1e6, 2.0 ** -20, 1), (0.5, 0.5, 2.0 ** 20, 0),
                                                (30.0, 10.0, 1.0, 1)])
def test_tables(lc, la, scale, colour):
    t = smx.adcensus_tables(_params(lc, la, scale, colour))
    want = ref.tables(lc, la, scale, colour)
    assert t.dtype == F32 and t.shape == (ref.TABLE_FLOATS,)
    # two libm's may round exp differently in the last double bit: one ulp of float32
    assert _ulps(t, want).max() <= 1, np.flatnonzero(_ulps(t, want) > 1)
    bits = t.view(np.uint32)
    assert bits[0] == 0 and bits[64] == 0                       # +0.0, not -0.0
    assert np.all(np.diff(t[:64]) >= 0) and np.all(np.diff(t[64:]) >= 0)
    assert np.all(t <= F32(scale))
    nz = t[t != 0]
    assert np.all(nz >= F32(2.0 ** -60)) and np.all(np.isfinite(nz)) and np.all(nz >= np.finfo(F32).tiny)
    assert np.all(t[1:64] > 0) and np.all(t[65:] > 0)           # only the two zeros are zero
    if not colour:
        assert np.all(t[64 + 256:] >= t[64 + 255]) and t[64 + 765] > 0     # filled beyond what gray images can index


def test_the_default_tables_keep_the_cost_inside_the_clamp_of_sgm():
    t = smx.adcensus_tables()
    assert t[:64].max() + t[64:].max() <= 255.0 and t[62] + t[64 + 255] > 200.0


def _bad_params():
    bad = []
    for v in (0.0, -1.0, float("nan"), float("inf"), -float("inf"), 1e6 * (1 + 1e-12), 1e7):
        bad += [_params(lc=v), _params(la=v)]
    for v in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 20 * (1 + 1e-12), 2.0 ** -20 * (1 - 1e-12)):
        bad.append(_params(scale=v))
    bad += [_params(colour=2), _params(colour=-1)]
    bad += [_params(rx=0), _params(rx=5), _params(ry=0), _params(ry=4), _params(th=0), _params(th=-3)]
    return bad


def test_argument_errors_do_not_need_a_gpu(lib):
    w, h = 6, 5
    img = np.zeros((2, h, w), np.uint8)
    rgb = np.zeros((2, h, w, 4), np.uint8)
    code = np.zeros((2, h, w), np.uint64)
    cost = np.zeros((2, 3, h, w), np.float32)
    tab = np.zeros(ref.TABLE_FLOATS, np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    good, goodc = _params(), _params(colour=1)

    def all_fail(fn, cases):
        for args in cases:
            p = C.byref(args[0]) if args[0] is not None else None
            assert fn(p, *args[1:]) == -1, args
            assert b"bad argument" in lib.smx_last_error()

    bad = [(p,) for p in _bad_params()] + [(None,)]
    # smx_adcensus_tables(p, tables)
    all_fail(lib.smx_adcensus_tables, [b + (P(tab),) for b in bad] + [(good, None)])
    assert not tab.any()
    # smx_dev_adcensus_tables(p, d_tables, stream)
    all_fail(lib.smx_dev_adcensus_tables, [b + (P(tab), None) for b in bad] + [(good, None, None)])
    # smx_dev_adcensus_cost_pair(p, d_tables, d_code, d_img_l, d_img_r, channels, d_cost_l, d_cost_r, w, h, dminl, dminr,
    #                            s_begin, s_end, stream)
    cl, cr, il, ir = P(cost[0]), P(cost[1]), P(img[0]), P(img[1])
    tail = (w, h, -2, 0, 0, 3, None)
    all_fail(lib.smx_dev_adcensus_cost_pair, [b + (P(tab), P(code), il, ir, 1, cl, cr) + tail for b in bad] + [
        (good, None, P(code), il, ir, 1, cl, cr) + tail, (good, P(tab), None, il, ir, 1, cl, cr) + tail,
        (good, P(tab), P(code), None, ir, 1, cl, cr) + tail, (good, P(tab), P(code), il, None, 1, cl, cr) + tail,
        (good, P(tab), P(code), il, ir, 1, None, None) + tail,
        (good, P(tab), P(code), il, ir, 1, cl, cr, 0, h, -2, 0, 0, 3, None),
        (good, P(tab), P(code), il, ir, 1, cl, cr, w, 0, -2, 0, 0, 3, None),
        (good, P(tab), P(code), il, ir, 1, cl, cr, -1, h, -2, 0, 0, 3, None),
        (good, P(tab), P(code), il, ir, 1, cl, cr, w, -1, -2, 0, 0, 3, None),
        (good, P(tab), P(code), il, ir, 1, cl, cr, w, h, -2, 0, 2, 1, None),
        (good, P(tab), P(code), il, ir, 1, cl, cr, w, h, -2, 0, -1, 3, None)] +
        # the channels follow `colour`
        [(good, P(tab), P(code), il, ir, ch, cl, cr) + tail for ch in (0, 2, 3, 4, -1)] +
        [(goodc, P(tab), P(code), P(rgb[0]), P(rgb[1]), ch, cl, cr) + tail for ch in (0, 1, 2, 5)])
    # smx_adcensus_cost(p, i1, i2, channels, cost, w, h, size_d, dmin)
    all_fail(lib.smx_adcensus_cost, [b + (il, ir, 1, cl, w, h, 3, -2) for b in bad] + [
        (good, None, ir, 1, cl, w, h, 3, -2), (good, il, None, 1, cl, w, h, 3, -2), (good, il, ir, 1, None, w, h, 3, -2),
        (good, il, ir, 1, cl, 0, h, 3, -2), (good, il, ir, 1, cl, w, 0, 3, -2), (good, il, ir, 1, cl, w, h, 0, -2),
        (good, il, ir, 1, cl, w, h, -1, -2), (good, il, ir, 3, cl, w, h, 3, -2), (good, il, ir, 4, cl, w, h, 3, -2),
        (goodc, P(rgb[0]), P(rgb[1]), 1, cl, w, h, 3, -2), (goodc, P(rgb[0]), P(rgb[1]), 2, cl, w, h, 3, -2)])
    assert not cost.any()
    with pytest.raises(smx.SmxError):
        smx.adcensus_cost(img[0], img[1], 0, 0)
    with pytest.raises(smx.SmxError):
        smx.adcensus_cost(img[0], img[1], 3, 0, _params(colour=1))        # gray images with the colour AD term
    with pytest.raises(smx.SmxError):
        smx.adcensus_tables(_params(lc=0.0))


def test_the_context_setter_needs_a_context(lib):
    assert lib.smx_ctx_set_adcensus(None, C.byref(_params())) == -1
    assert lib.smx_ctx_set_adcensus(None, None) == -1
    for p in _bad_params():
        assert lib.smx_ctx_set_adcensus(None, C.byref(p)) == -1
    # the separate setter leaves smx_ctx_set_cost's modes as they were
    assert lib.smx_ctx_set_cost(None, 2, None) == -1
    assert _lib.COST_MODES == {"reference": 0, "census": 1}


def test_refusals_of_the_python_layer():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError, match="cost must be"):       # (raised before anything is allocated: no device needed)
        PairPipeline(16, 8, 4, cost="bogus")
    with pytest.raises(ValueError, match="cost must be"):
        PairPipeline(16, 8, 4, cost="ad-census")
    with pytest.raises(ValueError, match="sharded"):
        ShardedPair(16, 8, 4, cost="adcensus")
    with pytest.raises(ValueError):
        smx.adcensus_cost(np.zeros((4, 5), np.uint8), np.zeros((4, 6), np.uint8), 2, 0)


# ---------------------------------------------------------------------------------------------
# what the feature is for
# ---------------------------------------------------------------------------------------------
def brightening_pattern():
    """A periodic pattern (period 8) in which every period is a little brighter than the one before: the local ORDER of the
    values repeats, their magnitudes do not.  The left image is the right one shifted so that the true label is -13."""
    P, w, h, D = 8, 96, 12, 24
    p = np.random.default_rng(3).permutation(P)
    row = lambda x: 9 * (x // P) + p[x % P] + 20
    x = np.arange(w)
    right = np.tile(row(x), (h, 1)).astype(np.uint8)
    left = np.tile(row(x - 13), (h, 1))                 # left[x] = right[x - 13]
    assert left.min() >= 0 and left.max() <= 255
    return left.astype(np.uint8), right, D, -(D - 1)


def _last_minimal_slice(v):
    return v.shape[0] - 1 - np.argmin(v[::-1], axis=0)


def test_the_census_cost_ties_a_period_away_and_adcensus_does_not():
    left, right, D, dminl = brightening_pattern()
    w = left.shape[1]
    inner = slice(D + 6, w - 6)                          # the interior columns D + 6 .. w - 7
    assert np.array_equal(left[:, 13:], right[:, :-13])
    cen = census_ref.census_cost(left, right, D, dminl)
    # 0 at the true label and one period to its right
    assert not cen[-13 - dminl][:, inner].any() and not cen[-5 - dminl][:, inner].any()
    won = _last_minimal_slice(cen)[:, inner] + dminl
    assert np.all(won != -13)                            # the last slice of equal costs wins: wrong on every interior pixel
    adc = ref.gray_cost(left, right, D, dminl)
    assert np.all(_last_minimal_slice(adc)[:, inner] + dminl == -13)
    assert np.all(adc[-13 - dminl][:, inner].view(np.uint32) == 0)                            # +0.0 at the true label
    # the library's tables give the same volume
    assert np.array_equal(ref.gray_cost(left, right, D, dminl, table=smx.adcensus_tables()).view(np.uint32), adc.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# a hand-worked case
# ---------------------------------------------------------------------------------------------
# tests/test_census_cpu.py HAND: window 3 x 3 (rx = ry = 1), th 8, the image against itself, labels -1 and 0
HAND = np.array([[5, 3, 8],
                 [1, 5, 9],
                 [7, 2, 5]], np.uint8)
# slice 0 (d = -1) compares x with x - 1: column 0 has its partner outside the image.  Hamming distances of the codes
# (test_census_cpu.py) and |I[y][x] - I[y][x - 1]|:
HAND_HC = [[None, 3, 2], [None, 3, 4], [None, 4, 3]]
HAND_AD = [[None, 2, 5], [None, 4, 4], [None, 5, 3]]


def test_reference_on_a_hand_worked_image():
    lc, la, scale = 4.0, 2.0, 10.0
    rho = lambda c, lam: F32(scale * (1.0 - math.exp(-c / lam)))
    c = ref.gray_cost(HAND, HAND, 2, -1, rx=1, ry=1, th=8, lambda_census=lc, lambda_ad=la, scale=scale)
    assert c.dtype == F32 and c.shape == (2, 3, 3)
    assert np.all(c[1].view(np.uint32) == 0)                                  # d = 0: both terms are +0.0
    for y in range(3):
        assert c[0, y, 0] == rho(8, lc) + rho(255, la)                         # outside: T[t] + T[64 + 255]
        for x in (1, 2):
            assert c[0, y, x] == rho(HAND_HC[y][x], lc) + rho(HAND_AD[y][x], la), (y, x)
    assert abs(float(rho(8, lc) + rho(255, la)) - 18.646647) < 4e-6           # 10 (1 - e^-2) + 10, within two ulp of f32
    # colour: three equal channels (and a fourth that is ignored) with the AD term over R, G, B: s triples, lambda_ad too
    rgba = np.stack([HAND, HAND, HAND, 255 - HAND], axis=-1)
    cc = ref.cost(rgba, rgba.copy(), HAND, HAND, 2, -1, rx=1, ry=1, th=8, lambda_census=lc, lambda_ad=la, scale=scale,
                  colour=1)
    for y in range(3):
        assert cc[0, y, 0] == rho(8, lc) + F32(scale * (1.0 - math.exp(-765 / (3 * la))))
        for x in (1, 2):
            assert cc[0, y, x] == rho(HAND_HC[y][x], lc) + F32(scale * (1.0 - math.exp(-3 * HAND_AD[y][x] / (3 * la))))
    # th 3 truncates the census half only; a sub-range is the slices of the whole volume
    c3 = ref.gray_cost(HAND, HAND, 2, -1, rx=1, ry=1, th=3, lambda_census=lc, lambda_ad=la, scale=scale)
    assert c3[0, 1, 2] == rho(3, lc) + rho(4, la) and c3[0, 1, 0] == rho(3, lc) + rho(255, la)
    full = ref.gray_cost(HAND, HAND[::-1].copy(), 5, -2, rx=1, ry=1, th=8)
    assert np.array_equal(ref.gray_cost(HAND, HAND[::-1].copy(), 5, -2, rx=1, ry=1, th=8, s_begin=1, s_end=4), full[1:4])
