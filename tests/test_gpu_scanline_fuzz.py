"""The seeded fuzz of the scan-line optimiser on the GPU: the twelve draws of tests/test_scanline_fuzz_cpu.py -- shape, label
ranges, parameters, guide kind, volume kind and the form of the call from one seeded rng -- through smx_dev_scanline_wta_pair on
guarded buffers with a poisoned workspace, bit for bit against tests/scanline_ref.py.  tests/test_scanline_fuzz_cpu.py
guarantees on the reference alone what the seeds hold.

A failure names its case: (BASE, seed) and the text of the draw reproduce it.
"""
import pytest

from stereo_matching_cuda_amd import _lib

from test_gpu_scanline import Call, _eq, _p, _uq_ref
from test_scanline_fuzz_cpu import BASE, SEEDS, reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(seed):
    c, want = reference(seed)
    name = f"base {BASE} seed {seed}: {c['text']}"
    views = {"both": (0, 1), "left": (0,), "right": (1,)}[c["form"]["views"]]
    costs = [c["cost"][v] if v in views else None for v in (0, 1)]
    call = Call(c["guides"][0], c["guides"][1], costs[0], costs[1], c["dmin"][0], c["dmin"][1], misalign=c["form"]["misalign"])
    outs = c["form"]["outs"]
    _lib.check(call.run(_p(**c["p"]), **outs))
    call.check_memory()
    for slot, v in enumerate(views):
        _eq(call.keys.numpy()[slot], want[v]["keys"], f"{name}: keys of view {v}")
        for key, g, w_ in (("agg", call.agg, want[v]["agg"]), ("nbr", call.nbr, want[v]["nbr"]), ("uq", call.uq, None)):
            if not outs[key]:
                g.check_untouched(f"{name}: d_{key} (not requested)")
            else:
                _eq(g.numpy()[slot], _uq_ref(want[v]["S"]) if w_ is None else w_, f"{name}: {key} of view {v}")
