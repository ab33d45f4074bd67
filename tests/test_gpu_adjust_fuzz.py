"""The seeded fuzz of the depth-discontinuity adjustment on the GPU: the twelve draws of tests/test_adjust_fuzz_cpu.py -- shape,
label range, parameters, map kind, volume kind, sub-pixel mode and the form of the call from one seeded rng -- through
smx_dev_discontinuity_adjust on guarded buffers, bit for bit against tests/adjust_ref.py.  tests/test_adjust_fuzz_cpu.py
guarantees on the reference alone what the seeds hold.

A failure names its case: (BASE, seed) and the text of the draw reproduce it.
"""
import pytest

from test_adjust_fuzz_cpu import BASE, SEEDS, reference
from test_gpu_adjust import MODES, Call, _bits, _p

pytestmark = pytest.mark.gpu
MODE_NAMES = {v: k for k, v in MODES.items()}


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(seed):
    c, want, wsub, _ = reference(seed)
    name = f"base {BASE} seed {seed}: {c['text']}"
    call = Call(c["disp"], c["vol"], c["dmin"], MODE_NAMES[c["mode"]], c["sub"], c["form"]["misalign"], c["form"]["in_place"])
    got = call.result(_p(**c["adjust"]))
    if c["mode"]:
        _bits(got[0], want, name)
        _bits(got[1], wsub, name + " sub")
    else:
        _bits(got, want, name)
