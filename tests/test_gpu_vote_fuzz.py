"""The seeded fuzz of region voting on the GPU: the twelve draws of tests/test_vote_fuzz_cpu.py -- shape, label range, parameters,
arms, guide kind, map kind and the form of the call from one seeded rng -- through smx_dev_cross_arms and smx_dev_region_vote
on guarded buffers, bit for bit against tests/vote_ref.py.  tests/test_vote_fuzz_cpu.py guarantees on the reference alone what
the seeds hold.

A failure names its case: (BASE, seed) and the text of the draw reproduce it.
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

from guarded import Guarded
from test_gpu_vote import Call, _bits, _p, _stream, _xp
from test_vote_fuzz_cpu import BASE, SEEDS, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(seed):
    c, arms, want, _, _ = reference(seed)
    name = f"base {BASE} seed {seed}: {c['text']}"
    h, w = c["h"], c["w"]
    # the arms on the device, from the drawn guide
    g = Guarded(c["guide"].nbytes, np.uint8, c["guide"].shape, plane=w * h, misalign=3).load(c["guide"])
    plane = Guarded(w * h * 4, np.uint8, (w * h * 4,), plane=w * h)
    _lib.check(smx.lib().smx_dev_cross_arms(C.byref(_xp(**c["arms"])), g.ptr, None, c["ch"], w, h, plane.ptr, _stream()))
    plane.check("d_arms")
    got_arms = plane.numpy().view(np.uint32).reshape(h, w)
    assert np.array_equal(got_arms, arms), name + ": arms"
    v = c["vote"]
    call = Call(c["disp"], got_arms, c["guide"], c["right"], c["dmin"], c["D"], c["d_lr"], c["form"]["misalign"], c["form"]["in_place"])
    p = _p(tau_s=v["tau_s"], tau_h_pct=v["tau_h_pct"], iterations=v["iterations"], interpolate=v["interpolate_"])
    _bits(call.result(p), want, name)
