"""Seeded fuzz of the ZNCC window cost on the GPU: a dozen draws of shape, window, label ranges, slice sub-range, views and
image kind from the generators of tests/fuzz_scenes.py, each bit for bit against tests/zncc_ref.py.  The shapes come from the
edge list of the cost kernel's tile (smx_zncc_geometry) on half of the draws.

Run on the GPU box:  python -m pytest tests/test_gpu_zncc_fuzz.py -m gpu -q
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import fuzz_scenes as fz
import zncc_ref as ref
from test_gpu_zncc import _cost_pair, _eq, _geometry, _zp

pytestmark = pytest.mark.gpu

BASE = 0x2ACC0000          # this stage's stream of seeds (fuzz_scenes.rng_of with an explicit base)
SEEDS = range(12)
CELLS = 1 << 19            # cells of a volume at the most: the reference stays quick


def draw(seed):
    rng = fz.rng_of("zncc", seed, BASE)
    cols, rows = _geometry()
    w, h = fz.dim(rng, (cols,), 1, 2 * cols + 9), fz.dim(rng, (rows,), 1, 2 * rows + 5)
    D = max(1, min(fz.dim(rng, (16,), 1, 40), CELLS // (w * h)))
    rx, ry = int(rng.integers(1, 5)), int(rng.integers(1, 5))
    dminl, dminr = fz.ranges_of(rng, D)
    s0, s1 = fz.sub_range(rng, D)
    views = ("both", "both", "left", "right")[int(rng.integers(0, 4))]
    Il, Ir = fz.pair(rng, seed % 4, w, h, D)
    return dict(w=w, h=h, D=D, rx=rx, ry=ry, dminl=dminl, dminr=dminr, s0=s0, s1=s1, views=views, Il=Il, Ir=Ir,
                text=f"{w}x{h}x{D} {fz.KINDS[seed % 4]} window {rx},{ry} dmin {dminl},{dminr} slices [{s0},{s1}) {views}")


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(seed):
    c = draw(seed)
    p = _zp(c["rx"], c["ry"])
    if c["s0"] == c["s1"]:
        # an empty range launches nothing and touches nothing
        import torch
        t = torch.full((1, c["h"], c["w"]), -7.0, device="cuda")
        d = torch.from_numpy(np.stack([c["Il"], c["Ir"]])).cuda()
        mom = torch.zeros((2, c["h"], c["w"]), dtype=torch.int64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(smx.lib().smx_dev_zncc_cost_pair(C.byref(p), C.c_void_p(mom.data_ptr()), C.c_void_p(d[0].data_ptr()),
                                                    C.c_void_p(d[1].data_ptr()), C.c_void_p(t.data_ptr()), None, c["w"], c["h"],
                                                    c["dminl"], c["dminr"], c["s0"], c["s1"], st))
        assert bool((t == -7.0).all()), c["text"]
        return
    gl, gr = _cost_pair(c["Il"], c["Ir"], p, c["dminl"], c["dminr"], c["s0"], c["s1"], left=c["views"] != "right",
                        right=c["views"] != "left")
    if gl is not None:
        _eq(gl, ref.zncc_cost(c["Il"], c["Ir"], c["D"], c["dminl"], c["rx"], c["ry"], c["s0"], c["s1"]), c["text"] + ": left")
    if gr is not None:
        _eq(gr, ref.zncc_cost(c["Ir"], c["Il"], c["D"], c["dminr"], c["rx"], c["ry"], c["s0"], c["s1"]), c["text"] + ": right")
