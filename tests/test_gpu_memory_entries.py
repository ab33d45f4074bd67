"""The guards of tests/guarded.py around the other device entries that write (include/smx.h): one test per entry, on the
shapes its own test uses, against what that test compares with.  Every output lies in a Guarded at a 256-byte boundary and at
the smallest alignment of its type past one (4 for f32, 1 for u8, 8 for the 64-bit codes), so a w*h u8 plane next to odd
addresses and planes that are no 8- or 16-byte multiples are covered; every input lies in one too and must be unchanged.

Run on the GPU box:  python -m pytest tests/test_gpu_memory_entries.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import census_ref
import subpix_ref
from guarded import Guarded
from test_gpu_parity import _eq
from test_gpu_wmf import _messy, _params as _wmf_params, _ref as _wmf_ref

pytestmark = pytest.mark.gpu

ALIGNED = [False, True]          # outputs on a 256-byte boundary / at the type's own alignment past one


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(dtype, shape, shifted, plane):
    dtype = np.dtype(dtype)
    return Guarded(int(np.prod(shape)) * dtype.itemsize, dtype, shape, misalign=dtype.itemsize if shifted else 0, plane=plane)


def _in(array, plane):
    a = np.ascontiguousarray(array)
    return Guarded(a.nbytes, a.dtype, a.shape, plane=plane).load(a)


def _done(outs, ins, what):
    for k, g in outs.items():
        g.check(f"{what} {k}")
    for k, g in ins.items():
        g.check_unchanged(f"{what} input {k}")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("w,h,size_d,dmin,s0,s1", [(33, 7, 5, -4, 2, 5), (2, 1, 3, -1, 1, 2), (65, 9, 40, -10, 3, 20)])
def test_cost_volume_on_a_sub_range(orc, w, h, size_d, dmin, s0, s1, shifted):
    rng = np.random.default_rng(w * 1000 + h)
    i1 = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    i2 = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    ins = dict(i1=_in(i1, w * h), i2=_in(i2, w * h))
    out = _out(np.float32, (s1 - s0, h, w), shifted, w * h)
    p = smx.default_params()
    _lib.check(smx.lib().smx_dev_cost_volume(C.byref(p), ins["i1"].ptr, ins["i2"].ptr, out.ptr, w, w, h, dmin, s0, s1, _stream()))
    _done(dict(cost=out), ins, "cost volume")
    _eq(out.numpy(), orc.cost_volume(i1, i2, size_d, dmin)[s0:s1], "cost")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("nplanes", [1, 2, 3])
@pytest.mark.parametrize("w,h", [(1, 1), (70, 1), (31, 63), (33, 65), (100, 130)])
def test_integral_of_several_planes(orc, w, h, nplanes, in_place, shifted):
    """nplanes independent planes, in place and out of place: the planes of a stack are scanned by one launch."""
    rng = np.random.default_rng(w + 7 * h + nplanes)
    img = rng.normal(size=(nplanes, h, w)).astype(np.float32)
    want = np.stack([orc.integral(p) for p in img])
    out = _out(np.float32, (nplanes, h, w), shifted, w * h)
    if in_place:
        out.load(img)
        ins, src = {}, out
    else:
        ins = dict(image=_in(img, w * h))
        src = ins["image"]
    _lib.check(smx.lib().smx_dev_integral(src.ptr, out.ptr, w, h, nplanes, _stream()))
    _done(dict(integral=out), ins, "integral")
    _eq(out.numpy(), want, f"integral of {nplanes} planes")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("shape", [(1, 1, 3), (7, 13, 3), (33, 65, 4)])
def test_rgb_to_grayscale(orc, shape, shifted):
    rgb = np.random.default_rng(5).integers(0, 256, size=shape, dtype=np.uint8)
    h, w, ch = shape
    ins = dict(rgb=_in(rgb, w * h))
    out = _out(np.uint8, (h, w), shifted, w * h)
    p = smx.default_params()
    _lib.check(smx.lib().smx_dev_rgb_to_grayscale(C.byref(p), ins["rgb"].ptr, w * h, ch, out.ptr, _stream()))
    _done(dict(gray=out), ins, "gray")
    _eq(out.numpy(), orc.gray(rgb), "gray")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("w,h,radius", [(1, 1, 9), (40, 7, 9), (63, 65, 4), (20, 20, 0)])
def test_filter(orc, w, h, radius, shifted):
    I = np.random.default_rng(w + h).integers(0, 256, size=(h, w), dtype=np.uint8)
    p = smx.default_params()
    p.radius = radius
    ins = dict(image=_in(I, w * h))
    outs = dict(mean=_out(np.uint8, (h, w), shifted, w * h), var=_out(np.float32, (h, w), shifted, w * h))
    _lib.check(smx.lib().smx_dev_filter(C.byref(p), ins["image"].ptr, w, h, outs["mean"].ptr, outs["var"].ptr, _stream()))
    _done(outs, ins, "filter")
    wm, wv = orc.filter(I, params=orc.Params.from_buffer_copy(bytes(p)))
    _eq(outs["mean"].numpy(), wm, "filter mean")
    _eq(outs["var"].numpy(), wv, "filter var")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("w", [300, 9000])
def test_finish_pair(orc, w, shifted):
    """The one-launch form (rows of at most 8192 pixels) and the three-kernel form behind it, on random keys."""
    h, size_d = 3, 5
    n = w * h
    rng = np.random.default_rng(w + h)
    dminl, dminr = -(size_d - 1), 0
    cost = (rng.random((2, h, w), dtype=np.float32) * 3).astype(np.float32)
    cost[rng.random((2, h, w)) < 0.05] = np.nan           # -> identity keys: the presets survive
    slices = rng.integers(0, size_d, size=(2, h, w))
    ins = dict(keys=_in(orc.pack_keys(cost, slices).reshape(2, h, w), n))
    outs = dict(best=_out(np.float32, (2, h, w), shifted, n), dmap=_out(np.float32, (2, h, w), shifted, n),
                occlusion=_out(np.float32, (h, w), shifted, n), filled=_out(np.float32, (h, w), shifted, n))
    p = smx.default_params()
    _lib.check(smx.lib().smx_dev_finish_pair(C.byref(p), ins["keys"].ptr, w, h, dminl, dminr, dminl - 100, float(dminl),
                                             outs["best"].ptr, outs["dmap"].ptr, outs["occlusion"].ptr, outs["filled"].ptr,
                                             _stream()))
    _done(outs, ins, "finish_pair")
    has = ~np.isnan(cost)
    best = np.where(has, cost, np.float32(np.frombuffer(b"\x7f\x7f\x7f\x7f", np.float32)[0])).astype(np.float32)
    dmin = np.array([dminl, dminr]).reshape(2, 1, 1)
    dmap = np.where(has, (dmin + slices).astype(np.float32), np.float32(0)).astype(np.float32)
    _eq(outs["best"].numpy(), best, "best")
    _eq(outs["dmap"].numpy(), dmap, "dmap")
    occ = orc.detect_occlusion(dmap[0], dmap[1], dminl - 100)
    _eq(outs["occlusion"].numpy(), occ, "occlusion")
    _eq(outs["filled"].numpy(), orc.fill_occlusion(occ, float(dminl)), "filled")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("mode", sorted(subpix_ref.MODES))
@pytest.mark.parametrize("w,h", [(2, 1), (37, 19), (153, 5)])
def test_subpixel_pair(orc, w, h, mode, shifted):
    """Keys, neighbour state and maps built from random volumes by tests/subpix_ref.py, some pixels without a winner."""
    n, size_d, dmins = w * h, 6, (-5, 0)
    rng = np.random.default_rng(w * 3 + h)
    keys, nbr, dmap, state = [], [], [], []
    for v in range(2):
        q = (rng.random((size_d, h, w), dtype=np.float32) * 2).astype(np.float32)
        q[:, rng.random((h, w)) < 0.05] = np.nan
        z, c0, lo, hi, last = subpix_ref.winners(q)
        keys.append(np.where(z >= 0, orc.pack_keys(c0, np.maximum(z, 0)), np.iinfo(np.int64).max))
        nbr.append(np.stack([lo, hi, last]))
        dmap.append(subpix_ref.dmap_of(z, c0, dmins[v]))
        state.append((z, c0, lo, hi))
    occ = orc.detect_occlusion(dmap[0], dmap[1], dmins[0] - 100)
    filled = orc.fill_occlusion(occ, float(dmins[0]))
    ins = dict(keys=_in(np.stack(keys), n), nbr=_in(np.stack(nbr), n), dmap=_in(np.stack(dmap), n), occlusion=_in(occ, n),
               filled=_in(filled, n))
    outs = dict(sub=_out(np.float32, (2, h, w), shifted, n), sub_filled=_out(np.float32, (h, w), shifted, n))
    _lib.check(smx.lib().smx_dev_subpixel_pair(subpix_ref.MODES[mode], ins["keys"].ptr, ins["nbr"].ptr, ins["dmap"].ptr,
                                               ins["occlusion"].ptr, ins["filled"].ptr, w, h, dmins[0], outs["sub"].ptr,
                                               outs["sub_filled"].ptr, _stream()))
    _done(outs, ins, "subpixel_pair")
    for v in range(2):
        sub, subf = subpix_ref.maps(subpix_ref.MODES[mode], *state[v], dmap[v], occ if v == 0 else None, filled, dmins[0])
        _eq(outs["sub"].numpy()[v], sub, f"view {v} sub")
        if v == 0:
            _eq(outs["sub_filled"].numpy(), subf, "sub_filled")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("h,w,radius", [(1, 1, 9), (3, 5, 15), (37, 70, 9), (9, 130, 4)])
def test_weighted_median(h, w, radius, shifted):
    rng = np.random.default_rng(h * 7 + w)
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = _messy(rng, h, w, -10, 24)
    sel = np.where(rng.random((h, w)) < 0.3, np.float32(-110), np.float32(-3)).astype(np.float32)
    p = _wmf_params(radius)
    ins = dict(guide=_in(g, w * h), disp=_in(d, w * h), select=_in(sel, w * h))
    for select in (None, sel):
        out = _out(np.float32, (h, w), shifted, w * h)
        _lib.check(smx.lib().smx_dev_weighted_median(C.byref(p), ins["guide"].ptr, ins["disp"].ptr,
                                                     ins["select"].ptr if select is not None else None, out.ptr, w, h, -10,
                                                     24, _stream()))
        _done(dict(out=out), ins, "weighted median")
        _eq(out.numpy(), _wmf_ref(g, d, -10, 24, select, p), f"{h}x{w} select={select is not None}")


@pytest.mark.parametrize("shifted", ALIGNED)
@pytest.mark.parametrize("nimages", [1, 2])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 9), (129, 70)])
def test_census(w, h, nimages, shifted):
    imgs = np.random.default_rng(5).integers(0, 256, size=(nimages, h, w), dtype=np.uint8)
    ins = dict(images=_in(imgs, w * h))
    out = _out(np.uint64, (nimages, h, w), shifted, w * h)
    p = smx.default_census_params()
    _lib.check(smx.lib().smx_dev_census(C.byref(p), ins["images"].ptr, out.ptr, w, h, nimages, _stream()))
    _done(dict(codes=out), ins, "census")
    got = out.numpy().view(np.uint64)
    for i in range(nimages):
        _eq(got[i], census_ref.census_transform(imgs[i]), f"codes of image {i}")
