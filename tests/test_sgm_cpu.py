"""Semi-global matching without a GPU: the numpy reference (tests/sgm_ref.py) against a scalar brute force written here
from the definition in include/smx.h, the properties that follow from the definition, the clamp, and the argument checks
of the library's host-only entry points."""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import sgm_ref


def brute_force(cost, p1, p2, paths):
    """S by the definition, one scalar at a time; every path walked from its own start pixel."""
    D, h, w = cost.shape
    Cv = [[[0] * w for _ in range(h)] for _ in range(D)]
    for d in range(D):
        for y in range(h):
            for x in range(w):
                c = float(cost[d, y, x])
                Cv[d][y][x] = (int(c) if c <= 255 else 255) if c >= 0 else 0
    S = np.zeros((D, h, w), np.int64)
    dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)][:paths]
    for dx, dy in dirs:
        for y0 in range(h):
            for x0 in range(w):
                if 0 <= y0 - dy < h and 0 <= x0 - dx < w:
                    continue                                   # not the start of a path
                x, y, prev = x0, y0, None
                while 0 <= x < w and 0 <= y < h:
                    cur = []
                    for d in range(D):
                        if prev is None:
                            cur.append(Cv[d][y][x])
                            continue
                        m = min(prev)
                        t = [prev[d], m + p2]
                        if d - 1 >= 0:
                            t.append(prev[d - 1] + p1)
                        if d + 1 < D:
                            t.append(prev[d + 1] + p1)
                        cur.append(Cv[d][y][x] + min(t) - m)
                    for d in range(D):
                        S[d, y, x] += cur[d]
                    prev = cur
                    x, y = x + dx, y + dy
    return S


def _volume(seed, D, h, w, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (D, h, w)).astype(np.float32)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("w,h,D", [(1, 1, 1), (1, 6, 3), (6, 1, 2), (4, 7, 1), (9, 7, 5), (7, 9, 4), (3, 3, 5)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_against_brute_force(paths, w, h, D, seed):
    cost = _volume(seed, D, h, w, 256 if seed else 63)
    for p1, p2 in ((10, 120), (0, 0), (7, 7), (3, 4095)):
        assert np.array_equal(sgm_ref.aggregate(cost, p1, p2, paths), brute_force(cost, p1, p2, paths)), (p1, p2)


@pytest.mark.parametrize("paths", [4, 8])
def test_zero_penalties_and_a_single_pixel_give_paths_times_c(paths):
    cost = _volume(3, 6, 8, 11)
    assert np.array_equal(sgm_ref.aggregate(cost, 0, 0, paths), paths * sgm_ref.clamp(cost))
    one = _volume(4, 9, 1, 1)
    assert np.array_equal(sgm_ref.aggregate(one, 10, 120, paths), paths * sgm_ref.clamp(one))


def test_path_costs_are_bounded_by_c_plus_p2():
    cost = _volume(5, 7, 9, 12)
    Cv = sgm_ref.clamp(cost)
    for p1, p2 in ((10, 120), (0, 33), (4095, 4095)):
        for dx, dy in sgm_ref.DIRS8:
            L = sgm_ref.path_costs(Cv, dx, dy, p1, p2)
            assert (L >= Cv).all() and (L <= Cv + p2).all()


@pytest.mark.parametrize("paths", [4, 8])
def test_constant_volume_names_the_last_slice(paths):
    cost = np.full((6, 5, 7), 17, np.float32)
    r = sgm_ref.outputs(cost, 10, 120, paths)
    assert (r["S"] == paths * 17).all()
    assert (r["z"] == 5).all()
    assert (r["keys"] == _lib.lib().smx_pack_key(float(paths * 17), 5)).all()
    assert np.isnan(r["nbr"][1]).all() and (r["nbr"][0] == paths * 17).all() and (r["nbr"][2] == paths * 17).all()


@pytest.mark.parametrize("paths", [4, 8])
def test_mirroring_in_x_mirrors_s(paths):
    cost = _volume(6, 5, 6, 9)
    S = sgm_ref.aggregate(cost, 10, 120, paths)
    assert np.array_equal(sgm_ref.aggregate(cost[:, :, ::-1], 10, 120, paths), S[:, :, ::-1])
    Cv = sgm_ref.clamp(cost)
    right = sgm_ref.path_costs(Cv, 1, 0, 10, 120)
    left_of_mirror = sgm_ref.path_costs(Cv[:, :, ::-1], -1, 0, 10, 120)
    assert np.array_equal(left_of_mirror[:, :, ::-1], right)


def test_clamp():
    v = np.array([-1, -0.0, 0.0, 0.99, 1, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e-30], np.float32)
    assert sgm_ref.clamp(v).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 255, 0, 255, 0, 255, 0]


def test_keys_match_the_library_packing():
    r = sgm_ref.outputs(_volume(7, 5, 4, 6), 10, 120, 8)
    L = _lib.lib()
    for (y, x), k in np.ndenumerate(r["keys"]):
        assert k == L.smx_pack_key(float(r["best"][y, x]), int(r["z"][y, x]))


# ---- host-only C ABI -------------------------------------------------------------------------------------------------
def _p(p1=10, p2=120, paths=8):
    p = _lib.SgmParams()
    p.p1, p.p2, p.paths = p1, p2, paths
    return p


def test_defaults():
    p = smx.default_sgm_params()
    assert (p.p1, p.p2, p.paths) == (10, 120, 8)
    assert isinstance(p, smx.SgmParams)


@pytest.mark.parametrize("p1,p2,paths,size_d", [(11, 10, 8, 4), (10, 4096, 8, 4), (-1, 10, 8, 4), (10, 120, 5, 4),
                                                (10, 120, 8, 257), (10, 120, 8, 0)])
def test_bad_arguments_are_refused_without_a_gpu(p1, p2, paths, size_d):
    L = smx.lib()
    buf = np.zeros(4 * 4 * 8, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p(p1, p2, paths)
    assert L.smx_dev_sgm_wta_pair(C.byref(p), ptr, ptr, 4, 4, size_d, ptr, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_last_error()
    assert L.smx_sgm_aggregate(C.byref(p), ptr, None, ptr, ptr, 4, 4, size_d, 0) == -1


def test_null_pointers_shapes_and_a_short_workspace_are_refused_without_a_gpu():
    L = smx.lib()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p()
    args = (4, 4, 4, ptr, None, None)
    assert L.smx_dev_sgm_wta_pair(None, ptr, ptr, *args, ptr, 1 << 40, None) == -1
    assert L.smx_dev_sgm_wta_pair(C.byref(p), None, None, *args, ptr, 1 << 40, None) == -1
    assert L.smx_dev_sgm_wta_pair(C.byref(p), ptr, ptr, 4, 4, 4, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_dev_sgm_wta_pair(C.byref(p), ptr, ptr, 0, 4, 4, ptr, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_dev_sgm_wta_pair(C.byref(p), ptr, ptr, 65536, 32768, 4, ptr, None, None, ptr, 1 << 40, None) == -1
    for l, r, nviews in ((ptr, ptr, 2), (ptr, None, 1), (None, ptr, 1)):
        need = L.smx_sgm_workspace_bytes(4, 4, 4, nviews)
        assert L.smx_dev_sgm_wta_pair(C.byref(p), l, r, *args, ptr, need - 1, None) == -3
        assert L.smx_dev_sgm_wta_pair(C.byref(p), l, r, *args, None, need, None) == -3
    with pytest.raises(ValueError):
        smx.sgm_aggregate(np.zeros((4, 4), np.float32))


def test_workspace_bytes():
    ws = smx.lib().smx_sgm_workspace_bytes
    assert ws(0, 5, 4, 1) == 0 and ws(5, 0, 4, 1) == 0 and ws(5, 5, 0, 1) == 0 and ws(5, 5, 257, 1) == 0
    assert ws(5, 5, 4, 0) == 0 and ws(5, 5, 4, 3) == 0 and ws(65536, 32768, 4, 1) == 0
    assert ws(5, 5, 256, 2) > 0
    # a u8 and a u16 plane of w*h*Dp cells per view, Dp = size_d rounded up to 64
    assert 3 * 1242 * 375 * 192 * 2 <= ws(1242, 375, 192, 2) <= 3 * 1242 * 375 * 192 * 2 + 4 * 256 + 255
    for w, h, d, v in ((7, 5, 9, 1), (64, 64, 64, 1), (129, 70, 70, 2), (33, 6, 255, 1)):
        assert ws(w + 1, h, d, v) >= ws(w, h, d, v) and ws(w, h + 1, d, v) >= ws(w, h, d, v)
        assert ws(w, h, d + 1, v) >= ws(w, h, d, v)
        if v == 1:
            assert ws(w, h, d, 2) > ws(w, h, d, 1)
    assert all(ws(9, 9, d + 1, 1) >= ws(9, 9, d, 1) for d in range(1, 256))


def test_pipeline_and_sharded_driver_refuse_what_they_do_not_take():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError, match="aggregation"):
        PairPipeline(16, 8, 4, aggregation="bogus")
    with pytest.raises(ValueError, match="semi-global"):
        ShardedPair(16, 8, 4, aggregation="sgm")
