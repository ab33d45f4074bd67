"""The weighted-median refinement without a GPU: the weight tables of the C-ABI, its argument checks (made before the
device is touched), and the numpy reference of tests/wmf_ref.py against a brute-force loop and its defining
properties."""
import ctypes as C
import math

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import wmf_ref


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _params(radius=9, sigma_s=9.0, sigma_c=25.5):
    p = _lib.WmfParams()
    p.radius, p.sigma_s, p.sigma_c = radius, sigma_s, sigma_c
    return p


def test_default_params(lib):
    p = smx.default_wmf_params()
    assert (p.radius, p.sigma_s, p.sigma_c) == (9, 9.0, 25.5)


@pytest.mark.parametrize("radius,sigma_s,sigma_c", [(9, 9.0, 25.5), (1, 1.0, 1.0), (15, 30.0, 4.0), (15, 1e9, 1e9),
                                                     (5, 0.05, 0.3), (3, 1e-200, 1e-200)])
def test_weight_tables_follow_the_formula(lib, radius, sigma_s, sigma_c):
    spatial, rng = smx.wmf_weights(_params(radius, sigma_s, sigma_c))
    assert spatial.shape == (2 * radius * radius + 1,) and rng.shape == (256,)
    ws, wc = wmf_ref.weight_tables(radius, sigma_s, sigma_c)
    assert spatial[0] == 1023 and rng[0] == 1023
    assert np.abs(spatial.astype(int) - ws.astype(int)).max() <= 1
    assert np.abs(rng.astype(int) - wc.astype(int)).max() <= 1
    assert np.all(np.diff(spatial.astype(int)) <= 0) and np.all(np.diff(rng.astype(int)) <= 0)
    if sigma_s >= 1e9:
        assert np.all(spatial == 1023) and np.all(rng == 1023)


def test_default_tables_exactly(lib):
    spatial, rng = smx.wmf_weights()
    for k in (0, 1, 17, 81, 162):
        assert spatial[k] == math.floor(1023 * math.exp(-k / 81.0) + 0.5)
    for t in (0, 1, 10, 25, 60, 255):
        assert rng[t] == math.floor(1023 * math.exp(-t * t / 650.25) + 0.5)


def _bad_params():
    return [_params(0), _params(16), _params(-3), _params(9, 0.0), _params(9, -1.0), _params(9, 9.0, 0.0),
            _params(9, math.inf), _params(9, 9.0, math.nan), _params(9, math.nan), _params(9, 9.0, -math.inf)]


def test_argument_errors_do_not_need_a_gpu(lib):
    w, h = 6, 5
    g = np.zeros((h, w), np.uint8)
    d = np.zeros((h, w), np.float32)
    o = np.zeros((h, w), np.float32)
    s = np.zeros((h, w), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    good = _params()
    cases = []
    for p in _bad_params():
        cases.append((p, P(g), P(d), P(s), P(o), w, h, 0, 4))
    cases += [
        (None, P(g), P(d), P(s), P(o), w, h, 0, 4),
        (good, None, P(d), P(s), P(o), w, h, 0, 4),
        (good, P(g), None, P(s), P(o), w, h, 0, 4),
        (good, P(g), P(d), P(s), None, w, h, 0, 4),
        (good, P(g), P(d), P(s), P(o), 0, h, 0, 4),
        (good, P(g), P(d), P(s), P(o), w, 0, 0, 4),
        (good, P(g), P(d), P(s), P(o), -1, h, 0, 4),
        (good, P(g), P(d), P(s), P(o), w, -7, 0, 4),
        (good, P(g), P(d), P(s), P(o), w, h, 0, 0),
        (good, P(g), P(d), P(s), P(o), w, h, 0, -1),
        (good, P(g), P(d), P(s), P(o), w, h, 0, 4097),
        (good, P(g), P(d), P(s), P(d), w, h, 0, 4),           # out == disp
        (good, P(g), P(d), None, P(d), w, h, 0, 4),
        (good, P(g), P(d), P(s), P(o), w, h, 2 ** 31 - 4, 4),  # dmin + size_d beyond int
    ]
    for args in cases:
        p = C.byref(args[0]) if args[0] is not None else None
        assert lib.smx_weighted_median(p, *args[1:]) == -1, args
        assert b"bad argument" in lib.smx_last_error()
        assert lib.smx_dev_weighted_median(p, *args[1:], None) == -1, args
        assert b"bad argument" in lib.smx_last_error()
    ws = np.zeros(2 * 16 * 16 + 1, np.uint16)
    wc = np.zeros(256, np.uint16)
    for p in _bad_params():
        assert lib.smx_wmf_weights(C.byref(p), P(ws), P(wc)) == -1
    assert lib.smx_wmf_weights(C.byref(good), None, P(wc)) == -1
    assert lib.smx_wmf_weights(C.byref(good), P(ws), None) == -1
    assert lib.smx_wmf_weights(None, P(ws), P(wc)) == -1
    with pytest.raises(smx.SmxError):
        smx.weighted_median(g, d, 0, 4097)


def _messy_map(rng, h, w, dmin, size_d, special=True):
    d = (dmin + rng.integers(0, size_d, size=(h, w))).astype(np.float32)
    if special:
        m = rng.random((h, w))
        d[m < 0.05] = np.nan
        d[(m >= 0.05) & (m < 0.08)] = np.inf
        d[(m >= 0.08) & (m < 0.10)] = -np.inf
        d[(m >= 0.10) & (m < 0.14)] = dmin - 100
        d[(m >= 0.14) & (m < 0.17)] += 0.5
        d[(m >= 0.17) & (m < 0.20)] = dmin + size_d            # one past the range
        d[(m >= 0.20) & (m < 0.22)] = -0.0
    return d


@pytest.mark.parametrize("h,w,dmin,size_d,radius,sig", [
    (7, 9, -5, 6, 2, (9.0, 25.5)), (5, 13, 3, 4, 3, (2.0, 10.0)), (1, 11, -2, 5, 2, (9.0, 25.5)),
    (9, 1, 0, 3, 4, (9.0, 25.5)), (3, 5, -15, 16, 15, (9.0, 25.5)), (6, 8, 0, 70, 2, (1.0, 3.0)),
    (8, 8, -1, 1, 1, (9.0, 25.5)),
])
def test_reference_equals_brute_force(h, w, dmin, size_d, radius, sig):
    rng = np.random.default_rng(h * 100 + w)
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = _messy_map(rng, h, w, dmin, size_d)
    ws, wc = wmf_ref.weight_tables(radius, *sig)
    sel = np.where(rng.random((h, w)) < 0.5, np.float32(dmin - 100), np.float32(dmin)).astype(np.float32)
    sel[0, 0] = np.nan
    for select in (None, sel):
        want = wmf_ref.brute_force(g, d, dmin, size_d, select, radius, ws, wc)
        for band in (1 << 22, size_d * w):                  # many bands and one
            got = wmf_ref.weighted_median(g, d, dmin, size_d, select, radius, ws, wc, band_elems=band)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_selection_rule():
    s = np.array([np.nan, np.inf, -np.inf, -16.0, -15.0, -15.5, -14.9, -115.0, -3e9, 0.0], np.float32)
    assert wmf_ref.selected(s, -15, s.shape).tolist() == [False, False, False, True, False, False, False, True,
                                                          True, False]


def test_constant_map_is_a_fixed_point():
    rng = np.random.default_rng(4)
    g = rng.integers(0, 256, size=(20, 30), dtype=np.uint8)
    d = np.full((20, 30), -7.0, np.float32)
    assert np.array_equal(wmf_ref.weighted_median(g, d, -15, 16, radius=9), d)


def test_flat_weights_give_the_lower_median_of_the_clipped_window():
    rng = np.random.default_rng(5)
    h, w, r = 9, 12, 3
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = rng.integers(-4, 6, size=(h, w)).astype(np.float32)
    ws, wc = wmf_ref.weight_tables(r, 1e9, 1e9)
    assert np.all(ws == 1023) and np.all(wc == 1023)
    got = wmf_ref.weighted_median(g, d, -4, 10, radius=r, spatial=ws, rng=wc)
    for y in range(h):
        for x in range(w):
            win = np.sort(d[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].ravel())
            assert got[y, x] == win[(win.size - 1) // 2]


def test_a_one_pixel_streak_is_removed():
    h, w = 15, 40
    g = np.full((h, w), 100, np.uint8)
    d = np.full((h, w), 5.0, np.float32)
    d[7, 10:30] = 9.0
    got = wmf_ref.weighted_median(g, d, 0, 16, radius=4)
    assert np.all(got == 5.0)
