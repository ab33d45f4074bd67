"""The census / Hamming matching cost without a GPU: defaults and the bit count of the C-ABI, its argument checks (made
before the device is touched), and the numpy reference of tests/census_ref.py on a hand-worked image and against its
defining property, the invariance under a strictly increasing change of one image's intensities."""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import census_ref as ref


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _params(rx=4, ry=3, th=62):
    p = _lib.CensusParams()
    p.rx, p.ry, p.th = rx, ry, th
    return p


def test_defaults_and_bits(lib):
    p = smx.default_census_params()
    assert (p.rx, p.ry, p.th) == ref.DEFAULTS == (4, 3, 62)
    for (rx, ry), bits in (((1, 1), 8), ((4, 1), 26), ((4, 3), 62), ((2, 3), 34)):
        assert lib.smx_census_bits(C.byref(_params(rx, ry))) == bits == ref.nbits(rx, ry)
    assert lib.smx_census_bits(None) == -1
    assert _lib.COST_MODES == {"reference": 0, "census": 1}


def _bad_params():
    return [_params(0), _params(5), _params(-1), _params(4, 0), _params(4, 4), _params(4, -2), _params(4, 3, 0),
            _params(4, 3, -5)]


def test_argument_errors_do_not_need_a_gpu(lib):
    w, h = 6, 5
    img = np.zeros((2, h, w), np.uint8)
    code = np.zeros((2, h, w), np.uint64)
    cost = np.zeros((2, 3, h, w), np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    good = _params()

    def all_fail(fn, cases):
        for args in cases:
            p = C.byref(args[0]) if args[0] is not None else None
            assert fn(p, *args[1:]) == -1, args
            assert b"bad argument" in lib.smx_last_error()

    for p in _bad_params():
        assert lib.smx_census_bits(C.byref(p)) == -1
    bad = [(p,) for p in _bad_params()] + [(None,)]
    # smx_dev_census(p, d_img, d_code, w, h, nimages, stream)
    all_fail(lib.smx_dev_census, [b + (P(img), P(code), w, h, 2, None) for b in bad] + [
        (good, None, P(code), w, h, 2, None), (good, P(img), None, w, h, 2, None),
        (good, P(img), P(code), 0, h, 2, None), (good, P(img), P(code), w, 0, 2, None),
        (good, P(img), P(code), -3, h, 2, None), (good, P(img), P(code), w, -1, 2, None),
        (good, P(img), P(code), w, h, 0, None), (good, P(img), P(code), w, h, -2, None)])
    # smx_dev_census_cost_pair(p, d_code, d_cost_l, d_cost_r, w, h, dminl, dminr, s_begin, s_end, stream)
    cl, cr = P(cost[0]), P(cost[1])
    all_fail(lib.smx_dev_census_cost_pair, [b + (P(code), cl, cr, w, h, -2, 0, 0, 3, None) for b in bad] + [
        (good, None, cl, cr, w, h, -2, 0, 0, 3, None), (good, P(code), None, None, w, h, -2, 0, 0, 3, None),
        (good, P(code), cl, cr, 0, h, -2, 0, 0, 3, None), (good, P(code), cl, cr, w, 0, -2, 0, 0, 3, None),
        (good, P(code), cl, cr, -1, h, -2, 0, 0, 3, None), (good, P(code), cl, cr, w, -1, -2, 0, 0, 3, None),
        (good, P(code), cl, cr, w, h, -2, 0, 2, 1, None), (good, P(code), cl, cr, w, h, -2, 0, -1, 3, None)])
    # smx_census_cost(p, i1, i2, cost, w, h, size_d, dmin)
    all_fail(lib.smx_census_cost, [b + (P(img[0]), P(img[1]), cl, w, h, 3, -2) for b in bad] + [
        (good, None, P(img[1]), cl, w, h, 3, -2), (good, P(img[0]), None, cl, w, h, 3, -2),
        (good, P(img[0]), P(img[1]), None, w, h, 3, -2), (good, P(img[0]), P(img[1]), cl, 0, h, 3, -2),
        (good, P(img[0]), P(img[1]), cl, w, 0, 3, -2), (good, P(img[0]), P(img[1]), cl, w, h, 0, -2),
        (good, P(img[0]), P(img[1]), cl, w, h, -1, -2)])
    # smx_ctx_set_cost(ctx, mode, census): no context without a device; a bad mode is refused either way
    for mode in (7, -1, 2):
        assert lib.smx_ctx_set_cost(None, mode, None) == -1
    assert lib.smx_ctx_set_cost(None, _lib.COST_MODES["census"], C.byref(good)) == -1
    with pytest.raises(smx.SmxError):
        smx.census_cost(img[0], img[1], 0, 0)
    with pytest.raises(smx.SmxError):
        smx.census_transform(img[0], _params(5))


# a 3 x 3 image, window 3 x 3 (rx = ry = 1): neighbours k = 0 .. 7 are (dy, dx) = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1)
# (1,0) (1,1), replicate clamp
HAND = np.array([[5, 3, 8],
                 [1, 5, 9],
                 [7, 2, 5]], np.uint8)
# e.g. the centre, 5: neighbours 5 3 8 1 9 7 2 5 -> smaller: k 1, 3, 6 -> 2 + 8 + 64; the corner (0, 0), 5: clamped
# neighbours 5 5 3 5 3 1 1 5 -> k 2, 4, 5, 6 -> 4 + 16 + 32 + 64
HAND_CODES = np.array([[116, 32, 41],
                       [0, 74, 239],
                       [151, 1, 40]], np.uint64)


def test_reference_on_a_hand_worked_image():
    assert np.array_equal(ref.census_transform(HAND, 1, 1), HAND_CODES)
    assert ref.popcount(np.array([0, 1, 74, 239, 2 ** 64 - 1, 2 ** 63], np.uint64)).tolist() == [0, 1, 3, 7, 64, 1]
    # the image against itself, labels -1 and 0, th 8: slice 1 (d = 0) is all zeros; slice 0 (d = -1) compares x with
    # x - 1 and holds t = 8 in column 0
    c = ref.census_cost(HAND, HAND, 2, -1, 1, 1, 8)
    assert c.dtype == np.float32 and c.shape == (2, 3, 3)
    assert not c[1].any()
    # 32 ^ 116 = 84 (3 bits), 41 ^ 32 = 9 (2); 74 ^ 0 (3), 239 ^ 74 = 165 (4); 1 ^ 151 = 150 (4), 40 ^ 1 = 41 (3)
    assert c[0].tolist() == [[8, 3, 2], [8, 3, 4], [8, 4, 3]]
    # th 3 truncates, th beyond nbits is nbits
    assert ref.census_cost(HAND, HAND, 2, -1, 1, 1, 3)[0].tolist() == [[3, 3, 2], [3, 3, 3], [3, 3, 3]]
    assert ref.census_cost(HAND, HAND, 1, 5, 1, 1, 99).tolist() == [[[8, 8, 8]] * 3]
    # a sub-range is the slices of the whole volume
    full = ref.census_cost(HAND, HAND[::-1].copy(), 5, -2, 1, 1, 8)
    assert np.array_equal(ref.census_cost(HAND, HAND[::-1].copy(), 5, -2, 1, 1, 8, 1, 4), full[1:4])


def test_ties_are_not_smaller():
    flat = np.full((4, 6), 9, np.uint8)
    assert not ref.census_transform(flat, 4, 3).any()
    two = np.zeros((4, 6), np.uint8)
    two[:, 3:] = 200
    code = ref.census_transform(two, 1, 1)
    assert not code[:, :3].any()                       # the low side sees nothing smaller
    assert code[1, 3] == (1 << 0) | (1 << 3) | (1 << 5) and code[1, 4] == 0


@pytest.mark.parametrize("rx,ry", [(1, 1), (4, 1), (2, 3), (4, 3)])
def test_reference_is_invariant_under_an_increasing_map(rx, ry):
    rng = np.random.default_rng(rx * 10 + ry)
    L = rng.integers(0, 128, size=(13, 31), dtype=np.uint8)
    R = rng.integers(0, 128, size=(13, 31), dtype=np.uint8)
    R[4:9, 5:20] = R[4:9, 6:21]                         # some equal neighbours
    R2 = (2 * R + 1).astype(np.uint8)
    assert R2.max() <= 255 and np.any(R2 != R)
    assert np.array_equal(ref.census_transform(R2, rx, ry), ref.census_transform(R, rx, ry))
    for dmin, D in ((-7, 8), (-2, 5)):
        a = ref.census_cost(L, R, D, dmin, rx, ry, 62)
        assert np.array_equal(ref.census_cost(L, R2, D, dmin, rx, ry, 62), a)
        assert len(np.unique(a)) > 4                   # the volume is not trivial
        assert np.array_equal(ref.census_cost(R2, L, D, dmin, rx, ry, 62), ref.census_cost(R, L, D, dmin, rx, ry, 62))


def test_pipeline_refuses_an_unknown_cost():
    from stereo_matching_cuda_amd.device import PairPipeline
    with pytest.raises(ValueError, match="cost must be"):       # (raised before anything is allocated: no device needed)
        PairPipeline(16, 8, 4, cost="bogus")
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError, match="census"):
        ShardedPair(16, 8, 4, cost="census")
