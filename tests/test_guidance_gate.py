"""The LDS gate of the comb walker's two-launch guidance (smx_agg_v5.h guid_block_width, through the test hook
smx_debug_guidance_block; no GPU): a workgroup of k_v5_guid_block keeps 2 planes x h rows x (bw + 19) columns of f32 and
1024 B of hand-over words in LDS, and the host takes the widest of 32 / 16 / 8 columns that fits the 160 KiB of a CU -- none:
the call keeps its three launches."""
import ctypes as C

import pytest

import stereo_matching_cuda_amd as smx

LDS = 160 * 1024


def _gate(h):
    L = smx.lib()
    L.smx_debug_guidance_block.restype = C.c_int
    L.smx_debug_guidance_block.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    bw, nbytes = C.c_int(-1), C.c_uint64(0)
    assert L.smx_debug_guidance_block(h, C.byref(bw), C.byref(nbytes)) == 0
    return bw.value, nbytes.value


def _bytes(h, bw):
    return 2 * h * (bw + 19) * 4 + 1024


@pytest.mark.parametrize("h,bw", [(1, 32), (288, 32), (375, 32), (399, 32), (400, 16), (581, 16), (582, 8), (753, 8),
                                  (754, 0), (2000, 0), (2160, 0)])
def test_block_width_at_its_boundaries(h, bw):
    got, nbytes = _gate(h)
    assert got == bw
    assert nbytes == (_bytes(h, bw) if bw else 0) and nbytes <= LDS
    if bw < 32:
        assert _bytes(h, 2 * bw if bw else 8) > LDS, "the next wider block must not fit"


def test_the_gate_is_monotone_and_never_over_the_limit():
    last = 32
    for h in range(1, 1200):
        bw, nbytes = _gate(h)
        assert bw in (32, 16, 8, 0) and bw <= last and nbytes <= LDS
        last = bw


def test_bad_arguments():
    L = smx.lib()
    L.smx_debug_guidance_block.restype = C.c_int
    L.smx_debug_guidance_block.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]
    bw = C.c_int(0)
    assert L.smx_debug_guidance_block(0, C.byref(bw), None) != 0
    assert L.smx_debug_guidance_block(10, None, None) != 0
    L.smx_debug_set_guidance_path.restype = C.c_int
    L.smx_debug_set_guidance_path.argtypes = [C.c_int]
    assert L.smx_debug_set_guidance_path(2) != 0 and L.smx_debug_set_guidance_path(-1) != 0
    assert L.smx_debug_set_guidance_path(0) == 0
