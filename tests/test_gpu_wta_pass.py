"""The WTA pass over materialised q planes (csrc/smx_wta.hip, k_wta<Order, EPL, NBR>) at the unroll boundary of every form,
with incoming keys and neighbour state: the pass takes a chunk's planes eight at a time with a scalar tail, so chunks of 1, 3, 7,
8, 9 and 17 slices are the tail alone, a full group, a group and one, two groups and one.  Through the public device entries
only; the reference is tests/subpix_ref.winners over the ORACLE's aggregated volumes, compared bit for bit.

Forms (which instantiation a call reaches: wta_launch in smx_wta.hip, aggregate_fused in smx_agg.hip):
  comb scratch, 4 per lane        path 5, no d_agg, 153 x 5: two strips, the last of one column; a ragged last row pair;
                                  456 quads per plane = two workgroups
  natural, 1 per lane             path 3, 153 x 5 (odd plane)
  natural, 2 per lane             path 3, 154 x 6 (even plane)
  natural over the caller's q     path 5 with d_agg, 154 x 6; and with d_agg 4 bytes off an 8-byte boundary: 1 per lane
  the gated pair                  cost volumes with one value the comb walker's check refuses: natural, gate_nonzero = 1 runs;
                                  clean volumes: comb, gate_nonzero = 0 runs

Run on the GPU box:  python -m pytest tests -m gpu -q -k wta_pass
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import subpix_ref as ref
from test_gpu_subpix import _Path, _check_state, _eq, _pipe

pytestmark = pytest.mark.gpu

D = 17
DMINL, DMINR = -(D - 1), 2
CHUNKS = [1, 7, 9, 17]                      # slices per launch: launches of 1 | 7, 7, 3 | 9, 8 | 17 slices
IDENT = np.iinfo(np.int64).max


def _volumes(w, h, seed):
    import oracle
    Il, Ir = synth.gen_pair(w, h, D, seed)
    want = oracle.stereo_pair(Il, Ir, D, dminl=DMINL, dminr=DMINR, want_agg=True)
    for a in (want["aggl"], want["aggr"]):
        a.setflags(write=False)
    return Il, Ir, (want["aggl"], want["aggr"])


@pytest.fixture(scope="module")
def odd():            # n = 765
    return _volumes(153, 5, 1535)


@pytest.fixture(scope="module")
def even():           # n = 924
    return _volumes(154, 6, 1546)


def _check_keys(keys, vols, name):
    """The packed keys of a plain pass against the reference winners of vols[v][D][h][w]."""
    import oracle
    for v in range(2):
        z, c0 = ref.winners(vols[v])[:2]
        want = np.where(z >= 0, oracle.pack_keys(c0, np.maximum(z, 0)), IDENT)
        _eq(keys[v], want, f"{name} view {v} keys")


def _check(pipe, vols, name):
    if pipe.subpixel:
        _check_state(pipe, vols, name=name)
    else:
        pipe.check_status()
        _check_keys(pipe.keys.cpu().numpy(), vols, name)
    if pipe.agg is not None:
        r = pipe.results()
        _eq(r["aggl"], vols[0], name + " aggl")
        _eq(r["aggr"], vols[1], name + " aggr")


def _run(case, path, sif, nbr, **kw):
    Il, Ir, vols = case
    with _Path(path):
        pipe = _pipe(Il, Ir, D, dminl=DMINL, dminr=DMINR, slices_in_flight=sif, subpixel="parabola" if nbr else None, **kw)
        assert smx.lib().smx_last_agg_path() == (2 if path == 3 else path)
        assert pipe.last_chunk() == (sif, -(-D // sif))
    return pipe


# ---------------------------------------------------------------------------------------------
# the forms at every chunk size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("sif", CHUNKS)
def test_comb_scratch(odd, sif, nbr):
    pipe = _run(odd, 5, sif, nbr)
    assert pipe.agg is None
    _check(pipe, odd[2], f"comb chunk {sif}")


@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("sif", CHUNKS)
def test_natural_one_per_lane(odd, sif, nbr):
    _check(_run(odd, 3, sif, nbr), odd[2], f"natural odd chunk {sif}")


@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("sif", CHUNKS)
def test_natural_two_per_lane(even, sif, nbr):
    _check(_run(even, 3, sif, nbr), even[2], f"natural even chunk {sif}")


@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "4-byte"])
@pytest.mark.parametrize("sif", CHUNKS)
def test_natural_over_the_callers_volume(even, sif, off, nbr):
    """The comb walker writes the caller's [slice][h][w] volume and the natural pass reads it back; a volume that starts 4 bytes
    off an 8-byte boundary cannot be read in 8-byte units: one pixel per lane on an even plane."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir, vols = even
    h, w = Il.shape
    with _Path(5):
        pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, slices_in_flight=sif, want_agg=True,
                            subpixel="parabola" if nbr else None)
        buf = torch.empty(pipe.agg.numel() + 2, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 8 == 0
        pipe.agg = buf[off:off + pipe.agg.numel()].view(pipe.agg.shape)
        assert pipe.agg.data_ptr() % 8 == 4 * off and (D * w * h) % 2 == 0
        pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
        assert smx.lib().smx_last_agg_path() == 5
    _check(pipe, vols, f"caller's volume +{4 * off} B chunk {sif}")


# ---------------------------------------------------------------------------------------------
# the gated pair behind a queued fall-back: exactly one of the two passes runs, in either state of the word
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cost_case():
    import oracle
    w, h = 160, 40                                  # (as tests/test_gpu_subpix.py::test_cost_volumes_with_the_queued_fallback)
    Il, Ir = synth.gen_pair(w, h, D, 3)
    cl = oracle.cost_volume(Il, Ir, D, DMINL)
    cr = oracle.cost_volume(Ir, Il, D, DMINR)

    def agg(cl, cr):
        return (oracle.guided_filter(Il, cl, DMINL, want_agg=True)[3], oracle.guided_filter(Ir, cr, DMINR, want_agg=True)[3])
    cases = {"clean": ((cl, cr), agg(cl, cr))}
    for name, s in (("first", 2), ("last", 15)):    # chunks of 7 slices: [0, 7), [7, 14), [14, 17)
        bad = cl.copy()
        bad[s, 7, 23] = -1.0                        # one value outside what the comb walker's check accepts
        cases[name] = ((bad, cr), agg(bad, cr))
    return Il, Ir, cases


@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("which,fell_back", [("first", 1), ("last", 1), ("clean", 0)])
def test_gated_pair(cost_case, which, fell_back, nbr):
    Il, Ir, cases = cost_case
    costs, vols = cases[which]
    pipe = _pipe(Il, Ir, D, dminl=DMINL, dminr=DMINR, costs=costs, slices_in_flight=7, subpixel="equiangular" if nbr else None)
    assert smx.lib().smx_last_agg_path() == 5
    rr = C.c_int(-1)
    _lib.check(smx.lib().smx_dev_agg_fallback(C.c_void_p(pipe.ws.data_ptr()), C.byref(rr)))
    assert rr.value == fell_back
    _check(pipe, vols, f"gated pair, {which}")


# ---------------------------------------------------------------------------------------------
# fresh: the first pass of a call ignores what the keys and the state hold; a later call takes them in
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbr", [False, True], ids=["plain", "nbr"])
@pytest.mark.parametrize("path", [5, 3], ids=["comb", "natural"])
@pytest.mark.parametrize("ranges", [((0, 17),), ((0, 9), (9, 17))], ids=["single", "split"])
def test_fresh_and_split_calls(odd, path, ranges, nbr):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir, vols = odd
    h, w = Il.shape
    L = smx.lib()
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, slices_in_flight=7, subpixel="parabola" if nbr else None)
    pipe.keys.fill_(0)                              # (loaded, a key of 0 would beat every winner of these volumes)
    if nbr:
        pipe.nbr.fill_(123.0)
    tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    with _Path(path):
        for i, (s0, s1) in enumerate(ranges):
            L.smx_set_keys_fresh(1 if i == 0 else 0)
            try:
                args = (pipe.w, pipe.h, pipe.dminl, pipe.dminr, s0, s1, p(pipe.keys), None, None, p(pipe.ws), pipe.ws_bytes)
                if nbr:
                    pipe._aggregate_call(L.smx_dev_aggregate_wta_pair_nbr, p(tl), p(tr), None, None, *args, p(pipe.nbr))
                else:
                    pipe._aggregate_call(L.smx_dev_aggregate_wta_pair, p(tl), p(tr), *args)
            finally:
                L.smx_set_keys_fresh(0)
            assert L.smx_last_agg_path() == (2 if path == 3 else path)
    pipe.finish()
    _check(pipe, vols, f"path {path} calls {ranges}")
