"""PatchMatch stereo without a GPU: the numpy reference (tests/patchmatch_ref.py) against the pieces of the contract that can be
stated on their own (include/smx.h above smx_pm_params), the host side of the library (table, hash, defaults, refusals before
any device call), and the demonstration on a slanted surface.

Demonstration (slanted_scene: 96 x 32, 16 labels from -15, true left disparity -1.5 - 0.08 x - 0.10 y, measured on the 2560
pixels of the columns >= 16, seeds 0 / 1; radius 4, gamma 10, max_slope 2, 6 iterations):

    matcher                           off by more than 0.5    off by more than 1
    oracle's plain pair (labels)          754 / 767               100 / 67
    plain pair + parabola fit             505 / 459                21 / 22
    PatchMatch reference, 6 iterations     13 / 22                  8 / 10

At 4 iterations the search has not converged on this scene (244 / 407 pixels off by more than 0.5), so the test runs 6.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import oracle
import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import patchmatch_ref as ref
import subpix_ref

F32 = np.float32
DEMO_ITERATIONS = 6
DEMO = {   # seed -> (plain, plain + parabola, PatchMatch): (pixels off by more than 0.5, pixels off by more than 1)
    0: ((754, 100), (505, 21), (13, 8)),
    1: ((767, 67), (459, 22), (22, 10)),
}


def default_cc():
    p = smx.default_params()
    return ref.cost_const(p.alpha, p.th_color, p.th_grad)


def ref_params(pm):
    return ref.PMParams(pm.radius, pm.gamma, pm.iterations, pm.max_slope, pm.seed)


def pm_params(**kw):
    p = smx.default_pm_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def random_pair(rng, h, w, shift=2):
    """two textured gray views, the right one the left one moved by `shift` columns plus noise"""
    base = rng.integers(0, 256, (h, w + 2 * abs(shift) + 2)).astype(np.int32)
    left = base[:, abs(shift):abs(shift) + w]
    right = base[:, abs(shift) + shift:abs(shift) + shift + w] + rng.integers(-3, 4, (h, w))
    return left.astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# the host side of the contract
# ---------------------------------------------------------------------------------------------
def test_defaults():
    p = smx.default_pm_params()
    assert (p.radius, p.gamma, p.iterations, p.max_slope, p.seed) == (8, 10.0, 4, 2.0, 0)


@pytest.mark.parametrize("gamma", [10.0, 0.5, 37.25])
def test_the_table_is_exp_in_double_rounded(gamma):
    tab = np.array(smx.pm_weights(pm_params(gamma=gamma)), F32)
    want = np.array([math.exp(-k / gamma) for k in range(256)], np.float64).astype(F32)
    assert np.array_equal(bits(tab), bits(want))
    assert np.array_equal(bits(tab), bits(ref.weights(gamma)))
    assert tab[0] == 1.0


PINNED = (0x642F30E0, 0xFB49E243, 0x312CECDC, 0xF81E1F7D, 0xDC5302DE, 0x8F43582A)


def test_the_mixer_is_pinned():
    """fmix32 of MurmurHash3 and the first values of the counter hash, as literals"""
    assert [int(v) for v in ref.fmix32(np.array([0, 1, 2, 0xFFFFFFFF], np.uint32))] == [0, 0x514E28B7, 0x30F4C306, 0x81F16F39]
    want = {(0, 0, 0, 0): PINNED[0], (0, 0, 0, 1): PINNED[1], (0, 1, 0, 0): PINNED[2], (0, 0, 1, 0): PINNED[3],
            (1, 0, 0, 0): PINNED[4], (0xFFFFFFFF, 1, 123456, 98): PINNED[5]}
    for key, v in want.items():
        assert int(ref.pm_hash(*key)) == v, key
        assert smx.pm_hash(*key) == v, key
    rng = np.random.default_rng(5)
    for key in rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64):
        key = [int(k) for k in key]
        assert smx.pm_hash(*key) == int(ref.pm_hash(*key))
    u = ref.uniform(0, 0, np.arange(4096, dtype=np.uint32), 0)
    assert u.dtype == F32 and u.min() >= 0.0 and u.max() < 1.0 and 0.45 < u.mean() < 0.55


def test_bad_parameters_are_refused_before_any_device_call():
    so = smx.lib()
    tab = (C.c_float * 256)()
    for kw in (dict(radius=-1), dict(radius=18), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=float("inf")),
               dict(gamma=float("nan")), dict(iterations=0), dict(iterations=17), dict(max_slope=-0.5), dict(max_slope=8.5),
               dict(max_slope=float("nan"))):
        assert so.smx_pm_weights(C.byref(pm_params(**kw)), tab) == -1, kw
        assert so.smx_patchmatch(C.byref(smx.default_params()), C.byref(pm_params(**kw)), tab, tab, 4, 4, 4, -3, 0, tab, tab, tab,
                                 tab) == -1, kw
        assert b"radius" in so.smx_last_error()
    for kw in (dict(radius=0), dict(radius=17), dict(iterations=16), dict(max_slope=0.0), dict(max_slope=8.0)):
        assert so.smx_pm_weights(C.byref(pm_params(**kw)), tab) == 0, kw
    pm = smx.default_pm_params()
    for w, h, d, dl, dr in ((0, 4, 4, 0, 0), (4, 0, 4, 0, 0), (4, 4, 0, 0, 0), (4, 4, 2 ** 20 + 1, 0, 0), (4, 4, 4, -2 ** 20 - 1, 0),
                            (4, 4, 4, 0, 2 ** 20 + 1), (2 ** 24, 1, 4, 0, 0), (2 ** 16, 2 ** 15, 4, 0, 0)):
        assert so.smx_patchmatch(C.byref(smx.default_params()), C.byref(pm), tab, tab, w, h, d, dl, dr, tab, tab, tab, tab) == -1
        assert so.smx_pm_plane_cost(C.byref(smx.default_params()), C.byref(pm), tab, tab, w, h, d, dl, dr, tab, tab) == -1
    assert so.smx_pm_workspace_bytes(0, 5) == 0 and so.smx_pm_workspace_bytes(2 ** 16, 2 ** 15) == 0
    assert so.smx_pm_workspace_bytes(7, 5) == 255 + 1024 + 40 * 35          # table | 2 views x 8 B | snapshot of 6 planes


# ---------------------------------------------------------------------------------------------
# the reference against the contract's separate statements
# ---------------------------------------------------------------------------------------------
def test_the_gradient_is_the_cost_volumes():
    rng = np.random.default_rng(1)
    for h, w in ((3, 2), (4, 3), (5, 17)):
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        assert np.array_equal(bits(ref.xgrad(img)), bits(oracle.xderiv(img)))
    assert np.array_equal(ref.xgrad(np.full((3, 1), 9, np.uint8)), np.zeros((3, 1), F32))


@pytest.mark.parametrize("dmin,other_first", [(-6, False), (0, True), (-2, False), (-3, True)])
def test_radius_0_fronto_parallel_planes_are_the_cost_volume(dmin, other_first):
    """planes (0, 0, d) at radius 0: the plane cost is the reference's cost cell, bit for bit, the border constant where x + d
    leaves the image included -- for the left view's labels (negative) and the right view's (from 0)"""
    rng = np.random.default_rng(7 + dmin)
    size_d, h, w = 7, 6, 19
    a, b = random_pair(rng, h, w, 2)
    own, other = (b, a) if other_first else (a, b)
    vol = oracle.cost_volume(own, other, size_d, dmin)
    cc = default_cc()
    border = int(bits(cc["border"]).ravel()[0])
    seen_border = False
    for z in range(size_d):
        planes = np.zeros((3, h, w), F32)
        planes[2] = dmin + z
        got = ref.plane_cost_map(own, other, dmin, size_d, ref.PMParams(radius=0), cc, planes)
        assert np.array_equal(bits(got), bits(vol[z])), z
        seen_border |= bool((bits(got) == border).any())
    assert seen_border


def test_a_recentred_plane_keeps_its_disparities():
    """the plane of pixel (nx, ny), re-centred at (x, y), has at (x, y) the disparity the neighbour's plane has there"""
    a, b, d0 = F32(0.25), F32(-0.5), F32(-7.0)          # (exact in f32: every step is)
    for (nx, ny), (x, y) in (((10, 4), (11, 4)), ((10, 4), (10, 9)), ((10, 4), (5, 4)), ((3, 9), (3, 4))):
        got = ref.recentre(np.array([a]), np.array([b]), np.array([d0]), np.array([x]), np.array([y]), np.array([nx]), np.array([ny]))
        assert got.dtype == F32 and got[0] == d0 + a * (x - nx) + b * (y - ny)
    # and through the search: after one pass with one colour frozen, a pixel that adopted its left neighbour's plane
    got = ref.recentre(np.array([F32(0.1)]), np.array([F32(0.3)]), np.array([F32(-2.0)]), np.array([6]), np.array([2]),
                       np.array([1]), np.array([2]))
    assert bits(got)[0] == bits(F32(F32(-2.0) + F32(F32(0.1) * F32(5.0))) + F32(F32(0.3) * F32(0.0)))


def test_refinement_steps():
    assert ref.refinement_steps(1) == []
    assert [float(s) for s in ref.refinement_steps(2)] == [0.5, 0.25, 0.125]
    assert len(ref.refinement_steps(16)) == 7 and len(ref.refinement_steps(2 ** 20)) <= ref.DRAWS_PER_ITERATION


@functools.lru_cache(maxsize=None)
def small_run(seed, max_slope=2.0):
    rng = np.random.default_rng(11)
    left, right = random_pair(rng, 9, 14, -2)
    return ref.patchmatch(left, right, 5, -4, 0, ref.PMParams(radius=2, iterations=2, max_slope=max_slope, seed=seed), default_cc())


def test_the_search_is_deterministic_and_follows_the_seed():
    a = small_run(3)
    small_run.cache_clear()
    b = small_run(3)
    c = small_run(4)
    for k in ("planes", "cost", "disp", "label"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    assert not np.array_equal(bits(a["planes"]), bits(c["planes"]))


def test_the_outputs_hang_together():
    r = small_run(3)
    left_right = ((-4, 0), (0, 4))
    for v, (lo, hi) in enumerate(left_right):
        d0 = r["planes"][v, 2]
        assert np.array_equal(bits(r["disp"][v]), bits(d0))
        assert d0.min() >= lo and d0.max() <= hi
        assert np.abs(r["planes"][v, :2]).max() <= 2.0
        assert np.array_equal(r["label"][v], np.clip(np.floor(d0 + F32(0.5)), lo, hi))
    flat = small_run(3, 0.0)
    assert not flat["planes"][:, :2].any()                # max_slope 0: the fronto-parallel search


# ---------------------------------------------------------------------------------------------
# the demonstration
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def demo(seed):
    left, right, truth = ref.slanted_scene(seed)
    plain = oracle.stereo_pair(left, right, ref.SCENE_D, dminl=ref.SCENE_DMINL, dminr=0, want_agg=True)
    z, c0, lo, hi, _ = subpix_ref.winners(plain["aggl"])
    sub, _ = subpix_ref.maps(subpix_ref.PARABOLA, z, c0, lo, hi, plain["dmapl"])
    pm = ref.patchmatch(left, right, ref.SCENE_D, ref.SCENE_DMINL, 0,
                        ref.PMParams(radius=4, gamma=10.0, iterations=DEMO_ITERATIONS, max_slope=2.0, seed=seed), default_cc())
    return tuple(ref.error_counts(m, truth) for m in (plain["dmapl"], sub, pm["disp"][0]))


@pytest.mark.parametrize("seed", [0, 1])
def test_slanted_surface(seed):
    plain, parabola, pm = demo(seed)
    print(f"seed {seed}: plain {plain}, plain + parabola {parabola}, PatchMatch {pm}")
    assert (plain, parabola, pm) == DEMO[seed]
    assert 10 * pm[0] <= plain[0]


def test_the_scene_is_what_the_issue_describes():
    left, right, truth = ref.slanted_scene(0)
    assert left.shape == right.shape == (32, 96) and left.dtype == np.uint8
    assert truth[0, 0] == -1.5 and abs(truth[31, 95] - (-1.5 - 0.08 * 95 - 0.10 * 31)) < 1e-12
    xs = np.arange(96)[None, :] + truth
    assert xs[:, ref.SCENE_X0:].min() >= 0 and truth.min() >= ref.SCENE_DMINL          # the match lies in the other image
    assert int(right.max()) - int(right.min()) > 128                                    # textured
