"""CPU-side checks of the sub-pixel refinement: the numpy reference (tests/subpix_ref.py) against a brute-force replay of the
kernels' state machine and against the fits' own properties, the host formula smx_subpixel_delta against the reference bit
for bit, and the argument errors of the new entry points (no GPU needed: they fail before any launch)."""
import ctypes as C
import os

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import subpix_ref as ref

F32 = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.SO_PATH):
        smx.build()
    return _lib.lib()


def _bits_eq(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(both, 0, a.view(np.uint32)), np.where(both, 0, b.view(np.uint32)))


def _messy_volume(rng, D, h, w):
    q = rng.integers(0, 6, size=(D, h, w)).astype(F32)          # many ties
    m = rng.random((D, h, w))
    q[m < 0.05] = np.nan
    q[(m >= 0.05) & (m < 0.07)] = np.inf
    q[(m >= 0.07) & (m < 0.09)] = -0.0
    q[(m >= 0.09) & (m < 0.12)] *= F32(-1)
    q[:, 0, 0] = np.nan                                           # a pixel without a winner
    return q


@pytest.mark.parametrize("chunk", [1, 2, 3, 7])
def test_reference_equals_the_state_machine(chunk):
    rng = np.random.default_rng(chunk)
    q = _messy_volume(rng, 11, 4, 5)
    z, c0, lo, hi, last = ref.winners(q)
    Z, LO, HI, LAST = ref.brute_state(q, [(0, 11)], chunk)
    assert np.array_equal(z, Z) and _bits_eq(lo, LO) and _bits_eq(hi, HI) and _bits_eq(last, LAST)


def test_reference_split_calls_and_fresh_start():
    rng = np.random.default_rng(5)
    q = _messy_volume(rng, 12, 3, 4)
    for k in (1, 5, 11):
        Z, LO, HI, _ = ref.brute_state(q, [(0, k), (k, 12)], 2)
        z, _, lo, hi, _ = ref.winners(q)
        assert np.array_equal(z, Z) and _bits_eq(lo, LO) and _bits_eq(hi, HI)
    # a fresh call that starts at slice 4: winners at 4 have no lo
    z, _, lo, hi, _ = ref.winners(q, 4, 9)
    Z, LO, HI, _ = ref.brute_state(q, [(4, 9)], 3)
    assert np.array_equal(z, Z) and _bits_eq(lo, LO) and _bits_eq(hi, HI)
    assert np.isnan(lo[z == 4]).all() and np.isnan(hi[z == 8]).all()


@pytest.mark.parametrize("mode", [1, 2])
def test_delta_is_bounded(mode):
    rng = np.random.default_rng(mode)
    q = (rng.random((64, 32, 32)) * rng.choice([1e-3, 1.0, 1e6], size=(64, 1, 1))).astype(F32)
    q[rng.random(q.shape) < 0.3] = F32(0.5)                       # ties
    z, c0, lo, hi, _ = ref.winners(q)
    d = ref.delta(mode, c0, lo, hi)
    assert np.all(np.abs(d) <= 0.5) and np.isfinite(d).all()
    a, b = lo - c0, hi - c0
    assert np.all(a[~np.isnan(a)] >= 0) and np.all(b[~np.isnan(b)] > 0)


@pytest.mark.parametrize("d0", [3.0, 3.25, 7.5 - 1e-3, 10.4])
def test_fits_recover_a_sampled_minimum(d0):
    d = np.arange(16, dtype=np.float64)
    for mode, f in ((1, (d - d0) ** 2), (2, np.abs(d - d0))):
        q = f.astype(F32)[:, None, None]
        z, c0, lo, hi, _ = ref.winners(q)
        got = F32(z[0, 0]) + ref.delta(mode, c0, lo, hi)[0, 0]
        assert abs(float(got) - d0) <= 4e-6 * max(1.0, d0), (mode, got, d0)


def test_winners_at_the_ends_get_no_offset():
    q = np.array([1, 2, 3, 4], F32)[:, None, None] * np.ones((1, 1, 2), F32)
    q[:, 0, 1] = q[::-1, 0, 1]
    z, c0, lo, hi, _ = ref.winners(q)
    assert list(z[0]) == [0, 3]
    assert np.all(ref.delta(1, c0, lo, hi) == 0) and np.all(ref.delta(2, c0, lo, hi) == 0)


def _host_delta(lib, mode, c0, lo, hi):
    f = lib.smx_subpixel_delta
    return np.array([f(mode, float(a), float(b), float(c)) for a, b, c in zip(c0.ravel(), lo.ravel(), hi.ravel())], F32)


@pytest.mark.parametrize("mode", [1, 2])
def test_host_delta_equals_the_reference(lib, mode):
    rng = np.random.default_rng(10 + mode)
    c0 = (rng.standard_normal(3000) * 10).astype(F32)
    lo = c0 + np.abs(rng.standard_normal(3000) * 10).astype(F32)
    hi = c0 + np.abs(rng.standard_normal(3000) * 10).astype(F32)
    edge = np.array([
        (1.0, 1.0, 2.0), (1.0, 2.0, 1.0), (1.0, 1.0, 1.0),        # a == 0, b == 0, both 0
        (0.0, 0.0, 1e-45), (1.0, np.inf, 2.0), (1.0, 2.0, np.inf), (np.inf, np.inf, np.inf),
        (1.0, np.nan, 2.0), (1.0, 2.0, np.nan), (np.nan, 1.0, 2.0), (-0.0, 0.0, 3.0), (3e38, 3.4e38, 3.4e38),
        (-3e38, 3e38, 3e38), (1.0, 1.0 + 2 ** -23, 3.0), (5.0, 3.0, 7.0)], F32)
    c0, lo, hi = (np.concatenate([x, edge[:, i]]) for i, x in enumerate((c0, lo, hi)))
    got = _host_delta(lib, mode, c0, lo, hi)
    assert _bits_eq(got, ref.delta(mode, c0, lo, hi))
    assert smx.subpixel_delta("parabola" if mode == 1 else "equiangular", 5.0, 7.0, 6.0) == \
        ref.delta(mode, F32(5), F32(7), F32(6))


def test_host_delta_bad_mode_and_python_mode_names(lib):
    assert lib.smx_subpixel_delta(0, 1.0, 3.0, 2.0) == 0.0
    assert lib.smx_subpixel_delta(3, 1.0, 3.0, 2.0) == 0.0
    with pytest.raises(ValueError):
        smx.subpixel_delta("cubic", 1.0, 3.0, 2.0)


def test_version_is_0_11(lib):
    assert b" 0.11 " in lib.smx_version()


def test_argument_errors_of_the_new_entries(lib):
    E = -1
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    P = C.byref(smx.default_params())
    sp = lib.smx_dev_subpixel_pair
    assert sp(0, p, p, p, p, p, 4, 4, 0, C.c_void_p(p.value + 16), None, None) == E        # mode 0
    assert sp(3, p, p, p, p, p, 4, 4, 0, C.c_void_p(p.value + 16), None, None) == E        # unknown mode
    assert sp(1, None, p, p, p, p, 4, 4, 0, C.c_void_p(p.value + 16), None, None) == E     # no keys
    assert sp(1, p, None, p, p, p, 4, 4, 0, C.c_void_p(p.value + 16), None, None) == E     # no state
    assert sp(1, p, p, None, p, p, 4, 4, 0, C.c_void_p(p.value + 16), None, None) == E     # no map
    assert sp(1, p, p, p, p, p, 4, 4, 0, None, None, None) == E                            # no output
    assert sp(2, p, p, p, p, p, 4, 4, 0, p, None, None) == E                               # d_sub == d_dmap
    assert sp(1, p, p, C.c_void_p(p.value + 8), None, None, 4, 4, 0, C.c_void_p(p.value + 16), p, None) == E
    assert sp(1, p, p, C.c_void_p(p.value + 8), p, p, 0, 4, 0, C.c_void_p(p.value + 16), None, None) == E  # w 0
    assert b"bad argument" in lib.smx_last_error()
    # the _nbr aggregation entries: d_nbr is required, the rest is checked like the plain calls
    assert lib.smx_dev_aggregate_wta_nbr(P, p, p, None, 8, 8, 0, 0, 4, p, None, None, p, 64, None, None) == E
    assert lib.smx_dev_aggregate_wta_pair_nbr(P, p, p, None, None, 8, 8, 0, 0, 0, 4, p, None, None, p, 64, None,
                                              None) == E
    assert lib.smx_dev_aggregate_wta_pair_nbr(P, p, p, p, None, 8, 8, 0, 0, 0, 4, p, None, None, p, 64, p, None) == E
    assert lib.smx_dev_aggregate_wta_nbr(P, None, p, None, 8, 8, 0, 0, 4, p, None, None, p, 64, p, None) == E
    assert lib.smx_dev_aggregate_wta_nbr(P, p, p, None, 8, 8, 0, 4, 2, p, None, None, p, 64, p, None) == E
    # context entries
    assert lib.smx_ctx_set_subpixel(None, 1) == E
    assert lib.smx_ctx_subpixel_maps(None, None, None, None) == E


def test_pipeline_refuses_unknown_modes_before_touching_the_gpu():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError):
        PairPipeline(8, 8, 4, subpixel="cubic")
    with pytest.raises(ValueError):
        ShardedPair(8, 8, 4, rank=0, world=2, subpixel="parabola")
