"""The comb walker's row pairs outside the image (smx_agg_v5.hip: rows1_out / rows2_out): a pair of a border band
whose two rows both lie above row 0 or behind row h - 1 takes the column sums only -- stage 1 puts -0 into tile 2 for them,
stage 2 stores nothing.  Bit-exact against the oracle, as tests/test_gpu_parity.py: the shapes here walk the count of such
pairs through all its values at the top and the bottom of an item, for both stages, both q layouts and both cost sources.

Band grids (rows per slot): stage 1 a/b rows 10 s - 9 .. 10 s in pairs (odd, even), stage 2 q rows 10 s - 38 .. 10 s - 29 in
pairs (even, odd).  Heights 21 .. 30 are every residue of h mod 10 (an odd height ends in a ragged stage-2 pair, an even one
in a ragged stage-1 pair); 1 .. 20 have bands that are outside at both ends at once and items whose stage-2 slots are all
border.  Width 40 is one strip; 200 is two: the hand-off record then carries the -0 rows to the right strip's hand-in and
row scan."""
import numpy as np
import pytest

import stereo_matching_cuda_amd as smx

pytestmark = pytest.mark.gpu

KEYS = ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")
HEIGHTS = list(range(21, 31)) + [1, 2, 9, 10, 11, 19, 20]
D = 4


def _eq(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _images(w, h, d, seed):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h, w + d), dtype=np.uint8)
    return np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, d // 2: d // 2 + w])


_WANT = {}


def _case(orc, w, h):
    """images and the oracle's answer for a shape: computed once, shared by the tests, never written to"""
    if (w, h) not in _WANT:
        Il, Ir = _images(w, h, D, 4100 + 31 * w + h)
        want = orc.stereo_pair(Il, Ir, D, want_cost=True, want_agg=True)
        for a in (Il, Ir, *want.values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _WANT[(w, h)] = (Il, Ir, want)
    return _WANT[(w, h)]


def _run(Il, Ir, d, want_agg, cost=None):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, d, want_agg=want_agg)
    dl, dr = torch.from_numpy(np.array(Il)).cuda(), torch.from_numpy(np.array(Ir)).cuda()
    smx.lib().smx_set_agg_path(5)
    try:
        if cost is None:
            pipe.aggregate(dl, dr)
        else:
            pipe.aggregate(dl, dr, torch.from_numpy(np.array(cost[0])).cuda(), torch.from_numpy(np.array(cost[1])).cuda())
        # (a plane of fewer than four costs cannot hold a 16-byte quad: the ring walker takes those volumes)
        assert smx.lib().smx_last_agg_path() == (5 if cost is None or w * h >= 4 else 2)
    finally:
        smx.lib().smx_set_agg_path(0)
    pipe.finish()
    pipe.check_status()
    return pipe


@pytest.mark.parametrize("w", [40, 200])
@pytest.mark.parametrize("h", HEIGHTS)
def test_costs_from_the_images(orc, w, h):
    Il, Ir, want = _case(orc, w, h)
    r = _run(Il, Ir, D, True).results()             # q into the caller's volume
    for k in KEYS + ("aggl", "aggr"):
        _eq(r[k], want[k], f"{w}x{h} volume {k}")
    r = _run(Il, Ir, D, False).results()            # q into the pair entry's own comb-ordered scratch
    for k in KEYS:
        _eq(r[k], want[k], f"{w}x{h} scratch {k}")


@pytest.mark.parametrize("w", [40, 200])
@pytest.mark.parametrize("h", HEIGHTS)
def test_materialised_cost_volume(orc, w, h):
    Il, Ir, want = _case(orc, w, h)
    cost = (want["costl"], want["costr"])
    r = _run(Il, Ir, D, True, cost).results()
    for k in KEYS + ("aggl", "aggr"):
        _eq(r[k], want[k], f"{w}x{h} volume {k}")
    r = _run(Il, Ir, D, False, cost).results()
    for k in KEYS:
        _eq(r[k], want[k], f"{w}x{h} scratch {k}")


def test_an_items_bottom_rows_share_slots_with_the_next_items_top_rows(orc):
    """300 x 29 with 280 disparities: 2 strips x 2 views x 280 slices = 1 120 items on at most 512 workgroups, period 6: a workgroup
    runs the outside pairs at the top of its next item (stage 1, front slots 0 and 1) in the very slots in which stage 2 runs the
    ones at the bottom of the item before."""
    import ctypes as C
    w, h, d = 300, 29, 280
    from stereo_matching_cuda_amd import _lib
    L = smx.lib()
    bands, q_last, period = C.c_int(), C.c_int(), C.c_int()
    assert C.CDLL(_lib.SO_PATH).smx_debug_v5_period(C.c_int(h), C.c_int(2), C.byref(bands), C.byref(q_last), C.byref(period)) == 0
    assert (q_last.value, period.value) == (6, 6) and 2 * 2 * d > 2 * 512
    Il, Ir = _images(w, h, d, 4099)
    want = orc.stereo_pair(Il, Ir, d)
    pipe = _run(Il, Ir, d, False)
    assert L.smx_dev_agg_status(C.c_void_p(pipe.ws.data_ptr())) == 0, L.smx_last_error().decode()
    r = pipe.results()
    for k in KEYS:
        _eq(r[k], want[k], k)
