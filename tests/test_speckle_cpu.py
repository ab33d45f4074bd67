"""The numpy reference of the speckle filter (tests/speckle_ref.py) against hand-written cases, against scipy's
connected_components where scipy imports, and on the oracle's Tsukuba map; and the argument checks of the library's
entries that need no GPU."""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import speckle_ref

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    both_nan = np.isnan(a) & np.isnan(b)
    assert np.array_equal(np.where(both_nan, 0, a.view(np.uint32)), np.where(both_nan, 0, b.view(np.uint32)))


def test_which_pixels_count():
    d = np.array([[NAN, INF, -INF, -115, -15, -15.9, -16, -0.0, 0.25, 3e9, -3e9, 3.4e38]], np.float32)
    want = [False, False, False, False, True, True, False, True, True, True, False, True]
    assert speckle_ref.counts(d, -15).tolist() == [want]
    # (int)-15.9 = -15 passes vmin -15; (int)-0.7 = 0 passes vmin 0 and -1.0 does not
    assert speckle_ref.counts(np.array([[-0.7, -1.0]], np.float32), 0).tolist() == [[True, False]]


def test_hand_written_components():
    d = np.array([[1, 1, 5, 5, 5],
                  [1, 9, 9, 5, 2],
                  [7, 9, 2, 2, 2]], np.float32)
    label, size = speckle_ref.components(d, 0, 0)
    assert label.tolist() == [[0, 0, 2, 2, 2], [0, 6, 6, 2, 9], [10, 6, 9, 9, 9]]
    assert size.tolist() == [[3, 3, 4, 4, 4], [3, 3, 3, 4, 4], [1, 3, 4, 4, 4]]
    out = speckle_ref.speckle_filter(d, 0, -1, max_size=3, max_diff=0)
    assert out.tolist() == [[-1, -1, 5, 5, 5], [-1, -1, -1, 5, 2], [-1, -1, 2, 2, 2]]
    _same(speckle_ref.speckle_filter(d, 0, -1, max_size=0, max_diff=0), d)
    assert np.all(speckle_ref.speckle_filter(d, 0, -1, max_size=4, max_diff=0) == -1)


def test_a_chain_is_one_component_although_its_ends_differ_by_two():
    d = np.array([[4, 5, 6, 8]], np.float32)
    label, size = speckle_ref.components(d, 0, 1)
    assert label.tolist() == [[0, 0, 0, 3]] and size.tolist() == [[3, 3, 3, 1]]
    # fractions: 0.5 apart joins at max_diff 0.5, 0.75 apart does not
    d = np.array([[1.0, 1.5, 2.25, 2.75]], np.float32)
    assert speckle_ref.components(d, 0, 0.5)[0].tolist() == [[0, 0, 2, 2]]


def test_pixels_that_do_not_count_separate_and_are_copied():
    d = np.array([[3, NAN, 3, -115, 3, INF, 3]], np.float32)
    label, size = speckle_ref.components(d, -15, 1)
    assert label.tolist() == [[0, -1, 2, -1, 4, -1, 6]] and size.tolist() == [[1, 0, 1, 0, 1, 0, 1]]
    out = speckle_ref.speckle_filter(d, -15, -115, max_size=5, max_diff=1)
    _same(out, np.array([[-115, NAN, -115, -115, -115, INF, -115]], np.float32))


def test_spiral_and_checkerboard():
    h = w = 21
    d = np.zeros((h, w), np.float32)
    y, x = np.mgrid[0:h, 0:w]
    d[(x + y) % 2 == 1] = 1
    assert int(speckle_ref.components(d, 0, 0)[1].max()) == 1
    assert int(speckle_ref.components(d, 0, 1)[1].min()) == h * w
    s = speckle_ref.spiral(h, w)
    label, size = speckle_ref.components(s, 0, 0)
    arm = s == 1
    assert arm[0, 0] and np.all(label[arm] == 0) and np.all(size[arm] == arm.sum()) and arm.sum() > h * w // 3
    for vertical in (True, False):
        c = speckle_ref.comb(h, w, vertical)
        label, size = speckle_ref.components(c, 0, 0)
        assert np.all(label[c == 1] == 0) and np.all(size[c == 1] == (c == 1).sum())
        assert np.all(size[c == 0] == h - 1 if vertical else size[c == 0] == w - 1)


def test_against_scipy_where_it_imports():
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        pytest.skip("scipy is not installed")
    rng = np.random.default_rng(5)
    for h, w, labels, md in ((37, 53, 4, 0), (64, 80, 3, 1), (20, 200, 6, 1), (50, 50, 2, 0)):
        d = rng.integers(0, labels, size=(h, w)).astype(np.float32)
        d[rng.random((h, w)) < 0.05] = NAN
        d[rng.random((h, w)) < 0.05] = -100
        a, b = speckle_ref.edges(d, 0, md)
        n = h * w
        _, comp = connected_components(coo_matrix((np.ones(a.size), (a, b)), shape=(n, n)), directed=False)
        label, size = speckle_ref.components(d, 0, md)
        c = speckle_ref.counts(d, 0).ravel()
        first = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))
        assert np.array_equal(label.ravel()[c], first[comp][c])
        assert np.array_equal(size.ravel()[c], np.bincount(comp[c], minlength=comp.max() + 1)[comp][c])
        assert np.all(label.ravel()[~c] == -1) and np.all(size.ravel()[~c] == 0)


def test_tsukuba_counts(tsukuba_oracle):
    occ = tsukuba_oracle["occlusion"]
    _, size = speckle_ref.components(occ, -15, 1)
    assert int(size.max()) == 61898
    for max_size, rewritten in ((200, 1531), (10, 232)):
        out = speckle_ref.speckle_filter(occ, -15, -115, max_size, 1)
        changed = out.view(np.uint32) != occ.view(np.uint32)
        assert int(changed.sum()) == rewritten
        assert np.all(out[changed] == -115) and np.all(speckle_ref.counts(occ, -15)[changed])


# ---------------------------------------------------------------------------------------------
# the library's argument checks: they answer before anything touches a device
# ---------------------------------------------------------------------------------------------
def _p(max_size=200, max_diff=1.0):
    p = _lib.SpeckleParams()
    p.max_size, p.max_diff = max_size, max_diff
    return p


def test_defaults_and_workspace_size():
    p = smx.default_speckle_params()
    assert (p.max_size, p.max_diff) == (200, 1.0)
    L = smx.lib()
    assert 8 * 1242 * 375 <= L.smx_speckle_workspace_bytes(1242, 375) <= 8 * 1242 * 375 + 256
    assert L.smx_speckle_workspace_bytes(0, 5) == 0 and L.smx_speckle_workspace_bytes(5, -1) == 0
    assert L.smx_speckle_workspace_bytes(65536, 32768) == 0          # w*h = 2^31
    tw, th = C.c_int(), C.c_int()
    assert L.smx_speckle_geometry(C.byref(tw), C.byref(th)) == 0 and (tw.value, th.value) == (64, 16)


@pytest.mark.parametrize("max_size,max_diff,w,h", [(-1, 1.0, 4, 4), (5, -0.5, 4, 4), (5, float("nan"), 4, 4),
                                                   (5, float("inf"), 4, 4), (5, 1.0, 0, 4), (5, 1.0, 4, 0),
                                                   (5, 1.0, 65536, 32768)])
def test_bad_arguments_are_refused_without_a_gpu(max_size, max_diff, w, h):
    L = smx.lib()
    buf = np.zeros(16, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p(max_size, max_diff)
    assert L.smx_speckle_filter(C.byref(p), ptr, ptr, w, h, 0.0, -100.0) == -1
    assert b"bad argument" in L.smx_last_error()
    assert L.smx_dev_speckle_filter(C.byref(p), ptr, ptr, w, h, 0.0, -100.0, ptr, 1 << 40, None) == -1


def test_null_pointers_and_a_short_workspace_are_refused_without_a_gpu():
    L = smx.lib()
    buf = np.zeros(16, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p()
    assert L.smx_speckle_filter(None, ptr, ptr, 4, 4, 0.0, -100.0) == -1
    assert L.smx_speckle_filter(C.byref(p), None, ptr, 4, 4, 0.0, -100.0) == -1
    assert L.smx_speckle_filter(C.byref(p), ptr, None, 4, 4, 0.0, -100.0) == -1
    need = L.smx_speckle_workspace_bytes(4, 4)
    assert L.smx_dev_speckle_filter(C.byref(p), ptr, ptr, 4, 4, 0.0, -100.0, ptr, need - 1, None) == -3
    assert L.smx_dev_speckle_filter(C.byref(p), ptr, ptr, 4, 4, 0.0, -100.0, None, need, None) == -3
    with pytest.raises(ValueError):
        smx.speckle_filter(np.zeros(5, np.float32), 0, -100)
