"""The comb walker's guidance statistics in two launches (k_v4_guid_rows, k_v5_guid_block: column prefix, statistics and
comb-ordered copies per block of 32 / 16 / 8 columns, integral images in LDS) against the three launches they replace
(k_v4_guid_rows, k_v4_guid_cols, k_v5_perm) and against the oracle, bit for bit: the mean images and the six maps of a pair.
Both forms are driven through the thread's test hook smx_debug_set_guidance_path; smx_debug_last_guidance_block reports what a
call ran with.

Shapes: widths around the block (32), the block and its halo (51) and the strip (152, 171 = strip + halo), one column, two
strips; heights around the window (19), the band (10) and the hand-over segment of the column prefix (32), and on either side
of the LDS gate of every block width (more than eight segments there: the round robin of a plane's waves wraps).
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx

pytestmark = pytest.mark.gpu

KEYS = ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")


def _hooks():
    L = smx.lib()
    L.smx_debug_set_guidance_path.restype = C.c_int
    L.smx_debug_set_guidance_path.argtypes = [C.c_int]
    L.smx_debug_last_guidance_block.restype = C.c_int
    L.smx_debug_last_guidance_block.argtypes = [C.POINTER(C.c_int)]
    return L


def _eq(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _pair(Il, Ir, D, guidance_path):
    """One pair on the comb walker; returns (results, columns per guidance block of the call: 0 = three launches)."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    L = _hooks()
    h, w = Il.shape
    pipe = PairPipeline(w, h, D)
    bw = C.c_int(-2)
    L.smx_set_agg_path(5)
    assert L.smx_debug_set_guidance_path(guidance_path) == 0
    try:
        pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
        assert L.smx_last_agg_path() == 5
        assert L.smx_debug_last_guidance_block(C.byref(bw)) == 0
    finally:
        L.smx_debug_set_guidance_path(0)
        L.smx_set_agg_path(0)
    return pipe.results(), bw.value


def _images(w, h, D):
    rng = np.random.default_rng(31 * w + 7 * h + D)
    base = rng.integers(0, 256, size=(h, w + D), dtype=np.uint8)
    return np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, D // 2: D // 2 + w])


def _check(orc, w, h, D, want_bw):
    Il, Ir = _images(w, h, D)
    want = orc.stereo_pair(Il, Ir, D)
    fused, bw = _pair(Il, Ir, D, 0)
    assert bw == want_bw, f"w={w} h={h}: the call chose a guidance block of {bw} columns, expected {want_bw}"
    three, bw3 = _pair(Il, Ir, D, 1)
    assert bw3 == 0, "smx_debug_set_guidance_path(1) keeps the three launches"
    for k in KEYS:
        _eq(fused[k], three[k], f"w={w} h={h} two launches vs three: {k}")
        _eq(fused[k], want[k], f"w={w} h={h} two launches vs oracle: {k}")
        _eq(three[k], want[k], f"w={w} h={h} three launches vs oracle: {k}")


@pytest.mark.parametrize("w", [2, 31, 32, 33, 51, 151, 152, 153, 171, 300])
def test_widths(orc, w):
    _check(orc, w, 23, 4, 32)


@pytest.mark.parametrize("h", [1, 2, 9, 19, 20, 21, 33, 70])
def test_heights(orc, h):
    _check(orc, 200, h, 5, 32)


# 2 planes x h rows x (bw + 19) columns x 4 B + 1024 B of hand-over words against the 160 KiB of a CU:
# bw = 32 up to h = 399, 16 up to 581, 8 up to 753, then the three launches
@pytest.mark.parametrize("w,h,bw", [(40, 399, 32), (40, 400, 16), (37, 581, 16), (37, 582, 8), (21, 753, 8), (21, 754, 0)])
def test_lds_gate(orc, w, h, bw):
    _check(orc, w, h, 2, bw)


# workgroups per column block (smx_agg_v5.h guid_block_split: 256 / (blocks x views), at most 2, eight row pairs each at least):
# 39 blocks x 2 views (the KITTI width) and 47 x 2 -> 2, 132 x 2 -> 1; the widths and heights above run with 2
@pytest.mark.parametrize("w,h", [(1242, 33), (1500, 33), (4200, 20)])
def test_workgroups_per_block(orc, w, h):
    _check(orc, w, h, 3, 32)
