"""The seeded fuzz of cross-scale aggregation on the GPU: shape (up to 70 x 50), label ranges, scales, lambda and the form of the
call from one seeded rng.  The combination pass runs on random volumes in guarded buffers, the context on a synthetic pair with
every level's volumes from plain pipelines; both bit for bit against tests/cscale_ref.py.

A failure names its case: (BASE, seed) and the text of the draw reproduce it.
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import cscale_ref as ref
import test_gpu_cscale as t

pytestmark = pytest.mark.gpu

BASE = 20141
SEEDS = range(8)


def draw(seed):
    rng = np.random.default_rng([BASE, seed])
    c = dict(w=int(rng.integers(2, 71)), h=int(rng.integers(1, 51)), size_d=int(rng.integers(1, 20)),
             dmins=(int(rng.integers(-40, 9)), int(rng.integers(-40, 9))), scales=int(rng.integers(1, 6)),
             lam=float(rng.choice([0.0, 0.1, 0.3, 1.0, 3.0])), form=t.FORMS[int(rng.integers(0, len(t.FORMS)))],
             misalign=int(rng.choice([0, 4, 8, 12])))
    c["text"] = ", ".join(f"{k} {v}" for k, v in c.items())
    return rng, c


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_combine(seed):
    rng, c = draw(seed)
    w, h, size_d, dmins = c["w"], c["h"], c["size_d"], c["dmins"]
    levels = [t._volumes(rng, w, h, d, size_d, c["scales"]) for d in dmins]
    wants = [t._want_view(levels[v], dmins[v], size_d, c["lam"]) for v in range(2)]
    print(f"base {BASE} seed {seed}: {c['text']}")
    t._call(levels, wants, w, h, dmins, size_d, t._params(c["scales"], c["lam"]), *c["form"], c["misalign"])


@pytest.mark.parametrize("seed", SEEDS[:4])
def test_fuzz_context(orc, seed):
    rng, c = draw(seed)
    w, h = max(c["w"], 16), c["h"]
    scales = c["scales"]
    while ref.level(w, h, 0, 1, scales - 1)[0] < 2:
        scales -= 1
    print(f"base {BASE} seed {seed}: {w} x {h}, scales {scales}, lambda {c['lam']}")
    gray = synth.gen_pair(w, h, t.D, seed)
    want = t._want_pair(orc, t._level_volumes(gray, None, w, h, "reference", "gray", scales), c["lam"])
    ctx = t._ctx(w, h, "reference", "gray")
    try:
        _lib.check(smx.lib().smx_ctx_set_cross_scale(ctx, C.byref(t._params(scales, c["lam"]))))
        rc, on = t._ctx_run(ctx, gray, None, w, h)
        _lib.check(rc)
        for k, n in t.CTX_NAMES:
            t.same(on[k], want[n], f"seed {seed} context {k}")
    finally:
        smx.lib().smx_destroy(ctx)
