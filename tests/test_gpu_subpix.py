"""Sub-pixel refinement on the GPU (smx_dev_aggregate_wta*_nbr, smx_dev_subpixel_pair, PairPipeline(subpixel=...), the
context and smx_main --subpixel), bit-exact against tests/subpix_ref.py.  Every neighbour run passes no d_agg, so the WTA
pass over the walker's own scratch (k_wta<Comb, 4, true> for the comb walker) is what is tested; the reference volume comes from a
separate run with want_agg, or from the oracle.

Run on the GPU box:  python -m pytest tests -m gpu -q -k subpix
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import subpix_ref as ref
from main_harness import binary  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["parabola", "equiangular"]


def _eq(a, b, name=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        both_nan = np.isnan(a) & np.isnan(b)
        a, b = a.view(np.uint32), b.view(np.uint32)
        a = np.where(both_nan, 0, a)
        b = np.where(both_nan, 0, b)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


class _Path:
    """smx_set_agg_path for the calling thread, restored afterwards."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        _lib.check(smx.lib().smx_set_agg_path(self.path))

    def __exit__(self, *a):
        smx.lib().smx_set_agg_path(0)


def _pipe(Il, Ir, D, dminl=None, dminr=0, params=None, costs=None, **kw):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, D, dminl=dminl, dminr=dminr, params=params, **kw)
    tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    if costs is not None:
        pipe.aggregate(tl, tr, torch.from_numpy(costs[0]).cuda(), torch.from_numpy(costs[1]).cuda())
        pipe.finish()
    else:
        pipe.run(tl, tr)
    return pipe


def _check_state(pipe, vols, s_begin=0, s_end=None, name=""):
    """keys, lo, hi and the maps of a sub-pixel pipeline against the reference over the volumes vols[v][D][h][w]."""
    r = pipe.results()
    keys = pipe.keys.cpu().numpy()
    nbr = pipe.nbr.cpu().numpy()
    mode = ref.MODES[pipe.subpixel]
    dmins = (pipe.dminl, pipe.dminr)
    subs = []
    for v in range(2):
        z, c0, lo, hi, last = ref.winners(vols[v], s_begin, s_end)
        has = z >= 0
        got_has = keys[v] != np.iinfo(np.int64).max
        assert np.array_equal(has, got_has), f"{name} view {v}: winners"
        assert np.array_equal(ref.dmap_of(z, c0, dmins[v]), r["dmapl" if v == 0 else "dmapr"]), f"{name} view {v}: dmap"
        _eq(nbr[v, 0], lo, f"{name} view {v} lo")
        _eq(nbr[v, 1], hi, f"{name} view {v} hi")
        _eq(nbr[v, 2], last, f"{name} view {v} last")
        sub, subf = ref.maps(mode, z, c0, lo, hi, r["dmapl" if v == 0 else "dmapr"],
                             r["occlusion"] if v == 0 else None, r["filled"], pipe.dminl)
        _eq(r["subpixl" if v == 0 else "subpixr"], sub, f"{name} view {v} sub")
        assert np.all(np.abs(sub - r["dmapl" if v == 0 else "dmapr"]) <= 0.5)
        if v == 0:
            _eq(r["subpix_filled"], subf, f"{name} sub_filled")
        subs.append(sub)
    return r


def _plain_and_agg(Il, Ir, D, **kw):
    p = _pipe(Il, Ir, D, want_agg=True, **kw)
    r = p.results()
    return r, (r["aggl"], r["aggr"])


# ---------------------------------------------------------------------------------------------
# Tsukuba against the oracle
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tsukuba():
    import oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", "tsukuba_golden.npz"))
    Il, Ir = g["image_left"], g["image_right"]
    want = oracle.stereo_pair(Il, Ir, 16, dminl=-15, dminr=0, want_agg=True)
    return Il, Ir, want


@pytest.mark.parametrize("mode", MODES)
def test_tsukuba_against_the_oracle(tsukuba, mode):
    Il, Ir, want = tsukuba
    pipe = _pipe(Il, Ir, 16, dminl=-15, subpixel=mode)
    assert pipe.agg is None
    r = _check_state(pipe, (want["aggl"], want["aggr"]), name="tsukuba")
    plain = _pipe(Il, Ir, 16, dminl=-15).results()
    assert "subpixl" not in plain
    for k, v in plain.items():                    # every existing output is unchanged
        _eq(r[k], v, k)
    for k in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled"):
        _eq(r[k], want[k], k)
    frac = r["subpix_filled"] - np.trunc(r["subpix_filled"])
    assert np.count_nonzero(frac) > r["filled"].size // 2      # the maps really are sub-pixel


# ---------------------------------------------------------------------------------------------
# every aggregation path, chunking, calls, shapes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,radius", [(5, 9), (3, 9), (1, 9), (0, 12), (4, 9)])
def test_every_path(path, radius):
    Il, Ir = synth.gen_pair(197, 43, 24, 7)
    p = smx.default_params()
    p.radius = radius
    kw = dict(dminl=-23, dminr=2, params=p, slices_in_flight=7, multi_kernel=path in (0, 1))
    with _Path(path):
        _, vols = _plain_and_agg(Il, Ir, 24, **kw)
        pipe = _pipe(Il, Ir, 24, subpixel="parabola", **kw)
        assert smx.lib().smx_last_agg_path() == (path if path in (1, 4, 5) else 2 if path == 3 else 1)
        _check_state(pipe, vols, name=f"path {path} r {radius}")


@pytest.mark.parametrize("bad", ["first", "last"])
def test_cost_volumes_with_the_queued_fallback(bad):
    Il, Ir = synth.gen_pair(160, 40, 12, 3)
    from stereo_matching_cuda_amd.device import PairPipeline
    import torch
    plain = PairPipeline(160, 40, 12)
    cl, cr = (t.cpu().numpy() for t in plain.cost_volumes(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()))
    sl = slice(0, 4) if bad == "first" else slice(8, 12)
    cl[sl][:, 5:9, 20:30] = -1.0                     # outside what the comb walker's check accepts: ring walker reruns
    cr[sl][:, 7, 3] = np.nan
    _, vols = _plain_and_agg(Il, Ir, 12, costs=(cl, cr), slices_in_flight=4)
    pipe = _pipe(Il, Ir, 12, costs=(cl, cr), slices_in_flight=4, subpixel="equiangular")
    rr = C.c_int(0)
    _lib.check(smx.lib().smx_dev_agg_fallback(C.c_void_p(pipe.ws.data_ptr()), C.byref(rr)))
    assert rr.value == 1
    _check_state(pipe, vols, name=f"fallback {bad}")
    # the good chunks alone: no fall-back, the comb walker's pass
    pipe = _pipe(Il, Ir, 12, costs=(np.abs(cl), np.nan_to_num(cr)), slices_in_flight=4, subpixel="parabola")
    _, vols = _plain_and_agg(Il, Ir, 12, costs=(np.abs(cl), np.nan_to_num(cr)), slices_in_flight=4)
    _check_state(pipe, vols, name="costs")


@pytest.mark.parametrize("D", [1, 2, 19])
def test_chunking_and_split_calls(D):
    import torch
    Il, Ir = synth.gen_pair(171, 23, D, 11)
    _, vols = _plain_and_agg(Il, Ir, D)
    for sif in sorted({1, 2, 7, D}):
        pipe = _pipe(Il, Ir, D, slices_in_flight=sif, subpixel="parabola")
        _check_state(pipe, vols, name=f"D {D} chunk {sif}")
    if D < 2:
        return
    # two calls [0, k) and [k, D) equal one call
    L = smx.lib()
    for k in (1, D // 2, D - 1):
        pipe = _pipe(Il, Ir, D, subpixel="equiangular")
        pipe.keys.fill_(0)
        pipe.nbr.fill_(123.0)
        tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for s0, s1, fresh in ((0, k, 1), (k, D, 0)):
            L.smx_set_keys_fresh(fresh)
            try:
                _lib.check(L.smx_dev_aggregate_wta_pair_nbr(
                    C.byref(pipe.params), C.c_void_p(tl.data_ptr()), C.c_void_p(tr.data_ptr()), None, None, pipe.w,
                    pipe.h, pipe.dminl, pipe.dminr, s0, s1, C.c_void_p(pipe.keys.data_ptr()), None, None,
                    C.c_void_p(pipe.ws.data_ptr()), pipe.ws_bytes, C.c_void_p(pipe.nbr.data_ptr()), st))
            finally:
                L.smx_set_keys_fresh(0)
        pipe.finish()
        _check_state(pipe, vols, name=f"split {k}")
    # a fresh call that starts at slice 3: winners at 3 have no lo
    if D > 4:
        pipe = _pipe(Il, Ir, D, s_begin=3, subpixel="parabola")
        _check_state(pipe, vols, 3, D, name="s_begin 3")
        z = ref.winners(vols[0], 3, D)[0]
        assert np.isnan(pipe.nbr[0, 0].cpu().numpy()[z == 3]).all() and (z == 3).any()


@pytest.mark.parametrize("w,h", [(2, 1), (3, 2), (2, 7), (37, 19), (153, 5), (305, 11), (457, 3)])
def test_edge_shapes(w, h):
    strip = C.c_int(0)
    _lib.check(smx.lib().smx_agg_geometry(9, C.byref(strip), None, None))
    assert strip.value == 152                            # 153, 305, 457: a last strip of one column
    Il, Ir = synth.gen_pair(w, h, 6, w * 31 + h)
    _, vols = _plain_and_agg(Il, Ir, 6, dminl=-5, dminr=1)
    pipe = _pipe(Il, Ir, 6, dminl=-5, dminr=1, subpixel="parabola")
    _check_state(pipe, vols, name=f"{w}x{h}")


# ---------------------------------------------------------------------------------------------
# context, streams, graphs
# ---------------------------------------------------------------------------------------------
def test_context(tsukuba):
    Il, Ir, want = tsukuba
    L = smx.lib()
    h, w = Il.shape
    n = w * h
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), w, h, 16, C.byref(ctx)))
    try:
        bufs = {k: np.empty(n, np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, -15, 0, C.byref(out)))
        sub = [np.empty(n, np.float32) for _ in range(3)]
        assert L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)) == -1      # that pair ran without it
        assert L.smx_ctx_set_subpixel(ctx, 3) == -1
        for mode in MODES:
            _lib.check(L.smx_ctx_set_subpixel(ctx, _lib.SUBPIX_MODES[mode]))
            _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, -15, 0, C.byref(out)))
            _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
            r = _pipe(Il, Ir, 16, dminl=-15, subpixel=mode).results()
            _eq(sub[0].reshape(h, w), r["subpixl"], "ctx sub_l")
            _eq(sub[1].reshape(h, w), r["subpixr"], "ctx sub_r")
            _eq(sub[2].reshape(h, w), r["subpix_filled"], "ctx sub_filled")
            for k, v in (("filled", "filled"), ("dmap_l", "dmapl"), ("occlusion", "occlusion")):
                _eq(bufs[k].reshape(h, w), want[v], k)
            assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -15, 0) == -1
        _lib.check(L.smx_ctx_set_subpixel(ctx, 0))
        _lib.check(L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -15, 0))
        _lib.check(L.smx_ctx_wait(ctx, None, C.byref(out)))
        _eq(bufs["filled"].reshape(h, w), want["filled"], "async filled")
    finally:
        L.smx_destroy(ctx)


def test_side_stream_and_graph(tsukuba):
    import torch
    Il, Ir, want = tsukuba
    expect = _pipe(Il, Ir, 16, dminl=-15, subpixel="parabola").results()
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, 16, dminl=-15, subpixel="parabola")
    tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.run(tl, tr)
    side.synchronize()
    r = pipe.results()
    for k in ("subpixl", "subpixr", "subpix_filled", "filled"):
        _eq(r[k], expect[k], "side stream " + k)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            pipe.run(tl, tr)
    torch.cuda.synchronize()
    pipe.sub.fill_(-1.0)
    pipe.sub_filled.fill_(-1.0)
    pipe.nbr.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    r = pipe.results()
    for k in ("subpixl", "subpixr", "subpix_filled", "filled"):
        _eq(r[k], expect[k], "graph " + k)


def test_kitti_pipeline():
    w, h, D = synth.SHAPES["kitti"]
    Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS["kitti"])
    _, vols = _plain_and_agg(Il, Ir, D)
    pipe = _pipe(Il, Ir, D, subpixel="parabola")
    _check_state(pipe, vols, name="kitti")


# ---------------------------------------------------------------------------------------------
# smx_main --subpixel
# ---------------------------------------------------------------------------------------------
OUTPUTS = ["image_left", "image_right", "image_mean_left", "image_mean_right", "best_costl",
           "best_costr", "cost_lminus15", "cost_rminus15", "occlu_mapl", "disparity_mapl",
           "disparity_mapr", "occlu_mapl_filled"]


def _stage(tmp_path):
    data = tmp_path / "data"
    data.mkdir()
    for n in ("tsukuba0", "tsukuba1"):
        (data / (n + ".png")).write_bytes(open(os.path.join(ROOT, "tests", "golden", "tsukuba", n + ".png"), "rb").read())
    return data


@pytest.mark.parametrize("mode", MODES)
def test_main_subpixel(binary, tsukuba, tmp_path, mode):
    PIL = pytest.importorskip("PIL.Image")
    Il, Ir, want = tsukuba
    data = _stage(tmp_path)
    pfm, png = tmp_path / "d.pfm", tmp_path / "d.png"
    r = subprocess.run([binary, "--subpixel", mode, "--pfm", str(pfm), "--png16", str(png)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    expect = _pipe(Il, Ir, 16, dminl=-15, subpixel=mode).results()["subpix_filled"]
    rest = pfm.read_bytes().split(b"\n", 3)[3]
    d = np.ascontiguousarray(np.frombuffer(rest, "<f4").reshape(288, 384)[::-1])
    _eq(d, -expect, "pfm")
    v = -expect * np.float32(256.0)
    want16 = np.clip(v, 0, 65535).astype(np.uint16)
    got16 = np.asarray(PIL.open(png)).astype(np.uint16)
    _eq(got16, want16, "png16")
    assert np.count_nonzero(got16 % 256) > 0
    for name in OUTPUTS:
        gold = open(os.path.join(ROOT, "tests", "golden", "tsukuba", name + ".png"), "rb").read()
        assert (data / (name + ".png")).read_bytes() == gold, name


@pytest.mark.parametrize("flags", [["--subpixel", "cubic"], ["--subpixel", "parabola", "--wmf", "all"],
                                   ["--subpixel", "parabola", "--ngpu", "1"],
                                   ["--subpixel", "parabola", "--fused", "--pairs", "3", "--pipeline"]])
def test_main_refuses(binary, tmp_path, flags):
    _stage(tmp_path)
    r = subprocess.run([binary] + flags, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--subpixel" in r.stderr, r.stdout + r.stderr
