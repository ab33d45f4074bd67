"""The HIP paths against the reference's OWN code, away from Tsukuba: every case recorded in tests/golden/ref_cases/ (by
oracle/ref_build.py, from host builds of the reference) through every aggregation path the library admits for its
parameters, bit for bit.  Reads only the committed fixtures -- never the reference, oracle/_ref or the oracle -- so it cannot
be empty on a machine without them.

Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import ctypes as C
import math

import numpy as np
import pytest

import ref_fixtures as rf
import stereo_matching_cuda_amd as smx
from oracle import ref_cases as rc
from test_agg_gate import hook

pytestmark = pytest.mark.gpu

MAPS = ("meanl", "meanr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")
RAN = {1: 1, 3: 2, 5: 5}           # what smx_last_agg_path() reports for a forced path (0: what the hook says)


def test_every_mode_has_recorded_cases():
    assert len(rf.names("pair")) >= 35 and len(rf.names("gf")) >= 4 and len(rf.names("occ")) >= 9 and len(rf.names("gray")) >= 2


@pytest.fixture(scope="module")
def so():
    smx.lib()                    # first: binds the library to torch's HIP runtime
    L = C.CDLL(smx._lib.SO_PATH)
    L.smx_debug_agg_path.restype = C.c_int
    L.smx_debug_agg_path.argtypes = [C.POINTER(smx.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.smx_last_error.restype = C.c_char_p
    return L


def _params(c):
    return rf.set_params(smx.default_params(), c["macros"])


def _admitted(so, p, w, h, nviews, use_cost):
    """[(forced path, path that runs)]: the default and every forced path agg_path_for answers for these arguments."""
    auto, err = hook(so, p, w, h, nviews, use_cost, 0)
    assert err is None, err
    runs = [(0, auto)]
    for forced in (1, 3, 5):
        ran, err = hook(so, p, w, h, nviews, use_cost, forced)
        if err is None:
            assert ran == RAN[forced]
            runs.append((forced, ran))
    return runs


def _device_pair(Il, Ir, D, path, **kw):
    """(like _device_pair of tests/test_gpu_parity.py; returns the pipeline too)"""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, D, multi_kernel=(path == 1), **kw)
    smx.lib().smx_set_agg_path(path)
    try:
        pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
        ran = smx.lib().smx_last_agg_path()
    finally:
        smx.lib().smx_set_agg_path(0)
    return pipe, pipe.results(), ran


def _ragged_chunk(D):
    """Slices per launch that leave a ragged last chunk (None where D has no such value)."""
    return next((k for k in range(3, D) if D % k), None) or next((k for k in range(2, D) if D % k), None)


@pytest.mark.parametrize("name", rf.names("pair"))
def test_pair_case_on_every_admitted_path(so, name):
    c, fx = rf.load(name)
    m, w, h = c["macros"], c["w"], c["h"]
    D, dminl, dminr = rc.size_d(m), m["D_MIN"], -m["D_MAX"]
    p = _params(c)
    inp = rf.inputs(c)
    Il, Ir = inp["left"], inp["right"]
    if c.get("channels", 1) >= 3:
        Il, Ir = smx.rgb_to_grayscale(Il, params=p), smx.rgb_to_grayscale(Ir, params=p)
    gray = {"grayl": Il, "grayr": Ir}
    runs = _admitted(so, p, w, h, 2, False)
    if m["RADIUS"] > 9:
        assert runs == [(0, 1), (1, 1)], runs
    if m["RADIUS"] == 9 and m["EPS"] >= 1.0:
        assert (5, 5) in runs, runs                   # the table's radius-9 cost parameters are inside the comb walker's gate
    for forced, want_ran in runs:
        _, r, ran = _device_pair(Il, Ir, D, forced, dminl=dminl, dminr=dminr, want_agg=True, params=p)
        assert ran == want_ran, (name, forced, ran, want_ran)
        seen = rf.compare(name, fx, dict(r, **gray), f"path {forced} (ran {ran})")
        rf.expect_all(fx, seen, but=("costl", "costr"))
    # one pass in chunks with a ragged last one, on the default path
    k = _ragged_chunk(D)
    if k is not None:
        pipe, r, ran = _device_pair(Il, Ir, D, 0, dminl=dminl, dminr=dminr, want_agg=True, params=p, slices_in_flight=k)
        assert ran == runs[0][1]
        if ran != 1:
            assert pipe.last_chunk() == (k, math.ceil(D / k)), (name, pipe.last_chunk())
        rf.expect_all(fx, rf.compare(name, fx, dict(r, **gray), f"chunks of {k}"), but=("costl", "costr"))
    # the host-pointer pair entry, with both materialised volumes
    r = smx.stereo_pair(Il, Ir, D, dminl=dminl, dminr=dminr, want_cost=True, want_agg=True, params=p)
    rf.expect_all(fx, rf.compare(name, fx, dict(r, **gray), "smx_stereo_pair"))


@pytest.mark.parametrize("name", rf.names("gf"))
def test_gf_case_host_and_device_entries(so, name):
    """compute_guided_filter on a supplied volume with supplied presets: the host-pointer stage call, then the device entry
    on the materialised volume (smx_dev_aggregate_wta: the comb walker's cost-source mode and, for costs outside its value
    check, its queued fall-back; the ring walker; the multi-kernel path) with the presets folded in by smx_dev_apply_keys."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    from test_gpu_parity import _fallback_ran
    c, fx = rf.load(name)
    w, h, D, dmin = c["w"], c["h"], c["size_d"], c["dmin"]
    p = _params(c)
    inp = rf.inputs(c)
    best, dmap = inp["best"].copy(), inp["dmap"].copy()
    mean, agg = smx.compute_guided_filter(inp["I"], inp["cost"], best, dmap, dmin, want_agg=True, params=p)
    rf.expect_all(fx, rf.compare(name, fx, {"best": best, "dmap": dmap, "mean": mean, "agg": agg}, "compute_guided_filter"))

    runs = _admitted(so, p, w, h, 1, True)
    assert {f for f, _ in runs} == {0, 1, 3, 5} and runs[0] == (0, 5), runs
    guide, cost = torch.from_numpy(inp["I"]).cuda(), torch.from_numpy(inp["cost"]).cuda()
    for forced, want_ran in runs:
        for sif in (None, 4):                                        # one launch; chunks of 4 with a ragged last one
            pipe = PairPipeline(w, h, D, dminl=dmin, want_agg=True, params=p, multi_kernel=(forced == 1), slices_in_flight=sif)
            smx.lib().smx_set_agg_path(forced)
            try:
                pipe.init_keys()
                pipe.aggregate_view(0, guide, guide, cost)
                assert smx.lib().smx_last_agg_path() == want_ran, (name, forced)
            finally:
                smx.lib().smx_set_agg_path(0)
            pipe.check_status()
            if want_ran == 5:
                assert _fallback_ran(pipe) == (name == "gf_odd_costs"), (name, forced, sif)
            b, d = torch.from_numpy(inp["best"]).cuda(), torch.from_numpy(inp["dmap"]).cuda()
            smx.check(smx.lib().smx_dev_apply_keys(C.c_void_p(pipe.keys[0].data_ptr()), w * h, dmin, C.c_void_p(b.data_ptr()),
                                                   C.c_void_p(d.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            got = {"best": b.cpu().numpy(), "dmap": d.cpu().numpy(), "mean": pipe.mean[0].cpu().numpy(),
                   "agg": pipe.agg[0].cpu().numpy()}
            rf.expect_all(fx, rf.compare(name, fx, got, f"device entry, path {forced} (ran {want_ran}), slices per launch {sif}"))


@pytest.mark.parametrize("name", rf.names("occ"))
def test_occ_case_host_stage_calls(name):
    c, fx = rf.load(name)
    p = _params(c)
    inp = rf.inputs(c)
    got, d = {}, inp["dl"]
    if "dr" in inp:
        d = got["occlusion"] = smx.detect_occlusion(d, inp["dr"], c["d_occlusion"], params=p)
    got["filled"] = smx.fill_occlusion(d, c["vmin"])
    rf.expect_all(fx, rf.compare(name, fx, got, "stage calls"))


@pytest.mark.parametrize("name", rf.names("gray"))
def test_gray_case_host_stage_call(name):
    c, fx = rf.load(name)
    rgb = rf.inputs(c)["rgb"].reshape(c["h"], c["w"], c["channels"])
    rf.expect_all(fx, rf.compare(name, fx, {"gray": smx.rgb_to_grayscale(rgb, params=_params(c))}, "rgb_to_grayscale"))
