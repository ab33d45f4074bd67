"""Seeded fuzz of smx_dev_tree_wta_pair against tests/tree_ref.py: twelve draws of tests/fuzz_scenes.py's generator for the
permeability filter's entry -- the tree filter takes the same call forms -- under a base of its own: shapes with edge sizes, the
four kinds of guides (noise, patches with and without noise, constant) at 1 / 3 / 4 channels, the four kinds of volumes (the
"special" ones carry NaN, infinities and huge values in many slices), the views, the filtered volumes nowhere / apart / in
place, the states, a workspace for c of the slices and the calling thread's bound on the slices per launch.  The drawn sigma is
the tree filter's.  The call is tests/test_gpu_tree.py's guarded one.

Run on the GPU box:  python -m pytest tests -m gpu -q -k tree_fuzz
"""
import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import fuzz_scenes as fs
import test_gpu_tree as tt
import tree_ref as ref

pytestmark = pytest.mark.gpu

BASE = 47000          # the committed seeds: BASE + 0 .. 11 (the bases of fuzz_scenes.py end at 43200 + 57)


@pytest.mark.parametrize("seed", range(fs.SEEDS))
def test_tree_fuzz(seed):
    d = fs.permeability(seed, base=BASE)
    c = tt.Case.__new__(tt.Case)
    c.w, c.h, c.size_d, c.ch, c.sigma = d["w"], d["h"], d["D"], d["ch"], d["sigma"]
    c.vols, c.guides = list(d["costs"]), list(d["guides"])
    c.trees = [ref.build(g) for g in c.guides]
    c.blobs = [ref.blob(t) for t in c.trees]
    c.wants = [tt._want_view(c.vols[v], c.trees[v], c.guides[v], c.sigma) for v in range(2)]
    c.name = f"seed {BASE}+{seed}: {d['text']} levels {[t['levels'] for t in c.trees]}"
    print(c.name)
    for v in range(2):          # the library builds the very tree the reference filters on
        assert np.array_equal(smx.tree_build(c.guides[v]), c.blobs[v]), c.name
    L = smx.lib()
    _lib.check(L.smx_set_max_slices_per_launch(d["bound"]))
    try:
        tt._call(c, d["views"], d["store"], d["nbr"], d["uq"], ws_slices=d["c"])
    finally:
        _lib.check(L.smx_set_max_slices_per_launch(0))
