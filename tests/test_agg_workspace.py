"""The documented workspace of the aggregation is enough, checked on the CPU.

include/smx.h promises that a call given nviews x smx_agg_workspace_bytes_for(p, w, h, n) runs n slices per launch and that
smx_agg_workspace_bytes(w, h, 1) per view is enough for any call.  The sizes and the chunk a call runs with derive from one
description of each workspace (AggLayout for the fused walkers, MultiLayout for the multi-kernel path, smx_agg.h); the hook
smx_debug_agg_chunk returns, from that layout alone, the chunk of a call -- or its error -- with the worst case of 255 bytes
lost to the 256-byte alignment of the caller's pointer.  No GPU: the hook is host arithmetic.
"""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib
from guarded import SMX_E_WS, min_workspace

SHAPES = [(1242, 375), (384, 288), (2964, 2000), (3840, 2160), (8192, 5460), (2, 1), (152, 10), (153, 11), (330, 25)]
SLICES = (1, 2, 7, 16, 192, 512)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        smx.build()
    _lib.lib()
    L = C.CDLL(_lib.SO_PATH)
    L.smx_debug_agg_chunk.restype = C.c_int
    L.smx_debug_agg_chunk.argtypes = [C.POINTER(_lib.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.c_uint64, C.c_int, C.POINTER(C.c_int)]
    L.smx_agg_workspace_bytes.restype = C.c_size_t
    L.smx_agg_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
    L.smx_agg_workspace_bytes_for.restype = C.c_size_t
    L.smx_agg_workspace_bytes_for.argtypes = [C.POINTER(_lib.Params), C.c_int, C.c_int, C.c_int]
    return L


def _shapes():
    rng = np.random.default_rng(31)
    return SHAPES + [(int(rng.integers(2, 3001)), int(rng.integers(1, 2001))) for _ in range(300)]


def _align256(x):
    return (x + 255) // 256 * 256


def _multi_kernel_chunk(w, h, cost, ws, n):
    """The multi-kernel path's rule, stated here on its own: behind the 255 lost bytes and the 256 of the status block, five
    planes of pb bytes and per chunk k volumes (T0, T1, A, B and, where the costs are built from the images, C), each rounded
    up to 256 bytes.  The call needs room for ten planes; its chunk is the largest c with 5 pb + k align256(4 w h c) <= avail,
    at most the slices of the call.  (align256(x) <= y for a whole number of 256-byte units y exactly when x <= y.)"""
    pb, k = _align256(4 * w * h), 4 if cost else 5
    avail = ws - 255 - 256
    if ws < 256 or avail < 10 * pb:
        return None
    return min((avail - 5 * pb) // k // 256 * 256 // (4 * w * h), n)


def test_documented_workspace_holds_the_slices_it_is_sized_for(so):
    out = C.c_int()

    def chunk(p, w, h, nviews, cost, own_q, forced, ws, n):
        """(chunk, 0) or (None, error code)"""
        rc = so.smx_debug_agg_chunk(C.byref(p), w, h, nviews, cost, own_q, forced, ws, n, C.byref(out))
        return (out.value, 0) if rc == 0 else (None, rc)

    params = {}
    for r in (0, 3, 9, 12):
        params[r] = smx.default_params()
        params[r].radius = r
    checked = 0
    for (w, h) in _shapes():
        for n, r in itertools.product(SLICES, (0, 3, 9)):
            p = params[r]
            ws_for = so.smx_agg_workspace_bytes_for(C.byref(p), w, h, n)
            ws_any = so.smx_agg_workspace_bytes(w, h, n)
            ws_one = so.smx_agg_workspace_bytes(w, h, 1)
            assert 0 < ws_for <= ws_any and ws_one <= ws_any
            for nviews, cost, own_q, forced in itertools.product((1, 2), (0, 1), (1, 0), (0, 3)):
                where = f"{w}x{h} n={n} radius={r} nviews={nviews} cost={cost} own_q={own_q} forced={forced}"
                args = (p, w, h, nviews, cost, own_q, forced)
                assert chunk(*args, nviews * ws_for, n) == (n, 0), where
                assert chunk(*args, nviews * ws_any, n) == (n, 0), where
                got, rc = chunk(*args, nviews * ws_one, n)
                assert rc == 0 and got >= 1, where
                # the smallest workspace (in 256-byte steps) that holds one slice: at most the documented size, not below the
                # planes every call writes (status words, two image planes [h][w + 8] of 4 B, per view (mean_I, 1/(var + eps))
                # of 8 B and two integrals of 4 B, own q planes of 4 B); one step below it the call reports SMX_E_WS
                assert chunk(*args, 0, n) == (None, SMX_E_WS), where
                hi = min_workspace(so, *args, n) // 256       # (the bisection: tests/guarded.py)
                written = 256 + 2 * (w + 8) * h * 4 + nviews * w * h * (16 + (4 if own_q else 0))
                assert hi * 256 >= written, where
                got, rc = chunk(*args, hi * 256, n)
                assert rc == 0 and got >= 1, where
                assert chunk(*args, hi * 256 - 256, n) == (None, SMX_E_WS), where
                checked += 1
            # the multi-kernel path: forced at this radius and, once per (shape, n), where auto mode takes it (radius 12)
            for p, forced in [(params[r], 1)] + ([(params[12], 0)] if r == 0 else []):
                ws_for = so.smx_agg_workspace_bytes_for(C.byref(p), w, h, n)
                assert ws_for <= ws_any and (forced == 1 or ws_for == ws_any)
                for nviews, cost in itertools.product((1, 2), (0, 1)):
                    where = f"{w}x{h} n={n} radius={p.radius} nviews={nviews} cost={cost} forced={forced} (multi-kernel)"
                    args = (p, w, h, nviews, cost, 1, forced)
                    assert chunk(*args, nviews * ws_any, n) == (n, 0), where
                    # (the views run one after the other in the same planes: the need does not double with nviews)
                    for ws in (nviews * ws_any, ws_any, ws_one, nviews * ws_one):
                        got, rc = chunk(*args, ws, n)
                        assert rc == 0 and got >= 1 and got == _multi_kernel_chunk(w, h, cost, ws, n), where
                    assert chunk(*args, 0, n) == (None, SMX_E_WS), where
                    hi = min_workspace(so, *args, n) // 256
                    assert hi * 256 == 512 + 10 * _align256(4 * w * h), where
                    got, rc = chunk(*args, hi * 256, n)
                    assert rc == 0 and got >= 1 and got == _multi_kernel_chunk(w, h, cost, hi * 256, n), where
                    assert chunk(*args, hi * 256 - 256, n) == (None, SMX_E_WS), where
                    assert _multi_kernel_chunk(w, h, cost, hi * 256 - 256, n) is None, where
                    checked += 1
    assert checked == len(_shapes()) * len(SLICES) * (3 * 16 + 3 * 4 + 4) and checked > 49600 * 4 // 3
