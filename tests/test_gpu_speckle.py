"""Speckle removal on the GPU (smx_speckle_filter / smx_dev_speckle_filter, PairPipeline(speckle=...), the context entry,
smx_main --speckle), bit for bit against the numpy reference of tests/speckle_ref.py.

Run on the GPU box:  python -m pytest tests -m gpu -q -k speckle
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import speckle_ref as ref
import subpix_ref
import wmf_ref
from main_harness import binary  # noqa: F401  (a fixture)
from guarded import Guarded
from test_gpu_wmf import _eq, _messy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    tw, th = C.c_int(), C.c_int()
    _lib.check(smx.lib().smx_speckle_geometry(C.byref(tw), C.byref(th)))
    return tw.value, th.value


T, U = _geometry()          # tile columns, tile rows


def _p(max_size=200, max_diff=1.0):
    p = _lib.SpeckleParams()
    p.max_size, p.max_diff = max_size, max_diff
    return p


def _check(d, vmin, new_val, max_size, max_diff, name=""):
    got = smx.speckle_filter(d, vmin, new_val, _p(max_size, max_diff))
    want = ref.speckle_filter(d, vmin, new_val, max_size, max_diff)
    _eq(got, want, f"{name} max_size {max_size} max_diff {max_diff}")
    return got


# ---------------------------------------------------------------------------------------------
# shapes around the tile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, T + 1), (U + 1, 1), (U - 1, T - 1), (U, T), (U + 1, T + 1), (33, 129)])
def test_shapes(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    d = rng.integers(0, 4, size=(h, w)).astype(np.float32)
    verdicts = set()
    for max_size in (0, 1, 7, w * h):
        got = _check(d, 0, -100, max_size, 0, f"{h}x{w}")
        verdicts |= set(np.unique(got == -100).tolist())
    assert verdicts == {False, True}
    _check(d, 0, -100, 7, 1, f"{h}x{w}")


# ---------------------------------------------------------------------------------------------
# structured maps: 5 x 5 tiles
# ---------------------------------------------------------------------------------------------
H5, W5 = 5 * U, 5 * T


def _structured():
    return ref.structured(H5, W5)          # (shared with tests/test_host_twins_cpu.py)


@pytest.mark.parametrize("name", ["constant", "checkerboard", "spiral", "comb down", "comb right", "ramp x", "ramp y",
                                  "chain"])
def test_structured_maps(name):
    d, cases = _structured()[name]
    for max_diff, largest in cases:
        _, size = ref.components(d, 0, max_diff)
        if largest is not None:
            assert int(size.max()) == largest, (name, max_diff)
        big = int(size.max())
        for max_size in (big - 1, big):       # the largest component stays, then goes
            got = _check(d, 0, -100, max_size, max_diff, name)
            assert bool(np.all(got == -100)) == (max_size == big)


# ---------------------------------------------------------------------------------------------
# the exact threshold, inside a tile and across a tile corner
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_exact_threshold(extra):
    k = 7
    d = np.zeros((2 * U, 2 * T), np.float32)
    inside = [(3, 5 + i) for i in range(k + extra - 2)] + [(4, 5), (5, 5)]
    # an S through the corner of the four tiles: both rows and both columns next to it
    corner = [(U - 1, T - 2), (U - 1, T - 1), (U - 1, T), (U, T), (U, T - 1), (U + 1, T - 1), (U + 1, T)][:k] + \
             [(U + 1, T + 1)] * extra
    assert len(set(inside)) == len(set(corner)) == k + extra
    for y, x in inside + corner:
        d[y, x] = 5
    got = _check(d, 0, -100, k, 0, "threshold")
    for blob in (inside, corner):
        vals = {float(got[y, x]) for y, x in blob}
        assert vals == ({-100.0} if extra == 0 else {5.0}), (extra, vals)
    assert np.all(got[d == 0] == 0)


# ---------------------------------------------------------------------------------------------
# messy values
# ---------------------------------------------------------------------------------------------
def test_messy_values():
    rng = np.random.default_rng(23)
    h, w, dmin, size_d = 3 * U + 5, 2 * T + 9, -10, 6
    d = _messy(rng, h, w, dmin, size_d)
    for max_size, max_diff in ((5, 1.0), (40, 0.0), (3, 0.25), (0, 1.0)):
        got = _check(d, dmin, dmin - 100, max_size, max_diff, "messy")
        idle = ~ref.counts(d, dmin)
        _eq(got[idle], d[idle], "pixels that do not count keep their bits")
    frac = (rng.integers(0, 8, size=(h, w)) * 0.25).astype(np.float32)
    for max_size in (6, 60):
        _check(frac, 0, -100, max_size, 0.5, "fractions")


# ---------------------------------------------------------------------------------------------
# the contract of the device entry
# ---------------------------------------------------------------------------------------------
def _dev(p, t_in, t_out, vmin, new_val, ws_ptr, ws_bytes, stream=None):
    import torch
    h, w = t_in.shape
    st = stream if stream is not None else torch.cuda.current_stream()
    return smx.lib().smx_dev_speckle_filter(C.byref(p), C.c_void_p(t_in.data_ptr()), C.c_void_p(t_out.data_ptr()), w, h,
                                            vmin, new_val, ws_ptr, ws_bytes, C.c_void_p(st.cuda_stream))


@pytest.fixture(scope="module")
def contract_map():
    rng = np.random.default_rng(77)
    h, w = 2 * U + 3, 2 * T + 7
    d = _messy(rng, h, w, 0, 3)
    return d, ref.speckle_filter(d, 0, -100, 9, 1)


def test_in_place_equals_out_of_place(contract_map):
    import torch
    d, want = contract_map
    h, w = d.shape
    need = smx.lib().smx_speckle_workspace_bytes(w, h)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    t_in = torch.from_numpy(d).cuda()
    t_out = torch.full_like(t_in, 7.0)
    assert _dev(_p(9, 1), t_in, t_out, 0, -100, C.c_void_p(ws.data_ptr()), need) == 0
    assert _dev(_p(9, 1), t_in, t_in, 0, -100, C.c_void_p(ws.data_ptr()), need) == 0
    torch.cuda.synchronize()
    _eq(t_out.cpu().numpy(), want, "out of place")
    _eq(t_in.cpu().numpy(), want, "in place")


@pytest.mark.parametrize("misalign", [0, 1, 255])
def test_memory_contract(contract_map, misalign):
    import torch
    d, want = contract_map
    h, w = d.shape
    n = w * h
    need = smx.lib().smx_speckle_workspace_bytes(w, h)
    t_in = Guarded(4 * n, np.float32, (h, w), plane=n).load(d)
    outs = []
    for fill in (0x00, 0xFF, 0xA5):        # the workspace may hold anything: three poisons, one answer
        out = Guarded(4 * n, np.float32, (h, w), misalign=4 * (misalign % 64), plane=n)
        ws = Guarded(need, np.uint8, (need,), misalign=misalign, fill=fill, plane=n)
        assert _dev(_p(9, 1), t_in.view, out.view, 0, -100, ws.ptr, need) == 0
        out.check("d_out")
        ws.check("d_ws")
        t_in.check_unchanged("d_disp")
        outs.append(out.numpy())
        _eq(outs[-1], want, f"poison {fill:#x}")
    # one byte short: SMX_E_WS and nothing is launched
    out = Guarded(4 * n, np.float32, (h, w), plane=n)
    ws = Guarded(need - 1, np.uint8, (need - 1,), misalign=misalign, plane=n)
    assert _dev(_p(9, 1), t_in.view, out.view, 0, -100, ws.ptr, need - 1) == -3
    out.check_untouched("d_out of a refused call")
    ws.check_untouched("d_ws of a refused call")


@pytest.mark.parametrize("max_size,max_diff", [(-1, 1.0), (3, -1.0), (3, float("nan")), (3, float("inf"))])
def test_bad_parameters(contract_map, max_size, max_diff):
    import torch
    d, _ = contract_map
    h, w = d.shape
    need = smx.lib().smx_speckle_workspace_bytes(w, h)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    t = torch.from_numpy(d).cuda()
    assert _dev(_p(max_size, max_diff), t, t, 0, -100, C.c_void_p(ws.data_ptr()), need) == -1
    assert smx.lib().smx_dev_speckle_filter(C.byref(_p()), C.c_void_p(t.data_ptr()), C.c_void_p(t.data_ptr()), 0, h, 0, -100,
                                            C.c_void_p(ws.data_ptr()), need, None) == -1
    torch.cuda.synchronize()
    _eq(t.cpu().numpy(), d, "a refused call writes nothing")
    with pytest.raises(smx.SmxError):
        smx.speckle_filter(d, 0, -100, _p(max_size, max_diff))


def test_graph_capture(contract_map):
    import torch
    d, want = contract_map
    h, w = d.shape
    need = smx.lib().smx_speckle_workspace_bytes(w, h)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    t_in = torch.from_numpy(d).cuda()
    t_out = torch.full_like(t_in, 7.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):       # one stream, one branch: four launches in a row
            assert _dev(_p(9, 1), t_in, t_out, 0, -100, C.c_void_p(ws.data_ptr()), need, s) == 0
    torch.cuda.synchronize()
    for _ in range(2):
        t_out.fill_(7.0)
        ws.fill_(0x3C)
        graph.replay()
        torch.cuda.synchronize()
        _eq(t_out.cpu().numpy(), want, "graph replay")


# ---------------------------------------------------------------------------------------------
# Tsukuba: the oracle's LR-checked map
# ---------------------------------------------------------------------------------------------
def test_tsukuba_counts(tsukuba_oracle):
    occ = tsukuba_oracle["occlusion"]
    for max_size, rewritten in ((200, 1531), (10, 232)):
        got = _check(occ, -15, -115, max_size, 1, "tsukuba")
        assert int((got.view(np.uint32) != occ.view(np.uint32)).sum()) == rewritten
    # the largest component has 61 898 pixels: it survives max_size 61 897 alone, and nothing survives 61 898
    valid = ref.counts(occ, -15)
    got = _check(occ, -15, -115, 61897, 1, "tsukuba")
    assert int((got[valid] != -115).sum()) == 61898
    got = _check(occ, -15, -115, 61898, 1, "tsukuba")
    assert np.all(got[valid] == -115)


# ---------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------
def _pipe(Il, Ir, D, dminl, **kw):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, D, dminl=dminl, **kw)
    pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
    return pipe


@pytest.fixture(scope="module")
def pairs(tsukuba_gray, tsukuba_oracle, orc):
    """name -> (Il, Ir, D, dminl, the oracle's maps, the results of the plain pipeline with its aggregated volumes)"""
    out = {"tsukuba": (tsukuba_gray[0], tsukuba_gray[1], 16, -15, tsukuba_oracle)}
    Il, Ir = synth.gen_pair(129, 70, 12, 4711)
    out["synthetic"] = (Il, Ir, 12, -11, orc.stereo_pair(Il, Ir, 12, dminl=-11, dminr=0))
    for k, (Il, Ir, D, dminl, want) in list(out.items()):
        plain = _pipe(Il, Ir, D, dminl, want_agg=True)
        assert plain.despeckled is None and plain.speckle_ws is None
        r = plain.results()
        assert "despeckled" not in r
        out[k] = (Il, Ir, D, dminl, want, r)
    return out


@pytest.mark.parametrize("name,max_size", [("tsukuba", 200), ("synthetic", 30)])
def test_pipeline(pairs, orc, name, max_size):
    Il, Ir, D, dminl, want, plain = pairs[name]
    pipe = _pipe(Il, Ir, D, dminl, speckle=_p(max_size, 1.0))
    r = pipe.results()
    desp = ref.speckle_filter(want["occlusion"], dminl, dminl - 100, max_size, 1.0)
    assert np.any(desp != want["occlusion"])                     # the filter changed something
    _eq(r["despeckled"], desp, "despeckled")
    _eq(r["filled"], orc.fill_occlusion(desp, dminl), "filled")
    for k in ("occlusion", "bestl", "bestr", "dmapl", "dmapr", "meanl", "meanr"):
        _eq(r[k], plain[k], k)
    pipe.despeckled.fill_(7.0)                                   # the per-stage finish honours the mode too
    pipe.filled.fill_(7.0)
    pipe.finish_per_call()
    again = pipe.results()
    for k in ("despeckled", "filled", "occlusion", "bestl", "bestr", "dmapl", "dmapr"):
        _eq(again[k], r[k], "finish_per_call " + k)
    if name == "tsukuba":                                        # True = the defaults
        _eq(_pipe(Il, Ir, D, dminl, speckle=True).results()["despeckled"], desp, "speckle=True")


def test_pipeline_with_wmf_and_subpixel(pairs, orc):
    Il, Ir, D, dminl, want, plain = pairs["synthetic"]
    desp = ref.speckle_filter(want["occlusion"], dminl, dminl - 100, 30, 1.0)
    filled = orc.fill_occlusion(desp, dminl)
    r = _pipe(Il, Ir, D, dminl, speckle=_p(30, 1.0), wmf="occluded").results()
    p = smx.default_wmf_params()
    ws, wc = smx.wmf_weights(p)
    _eq(r["refined"], wmf_ref.weighted_median(Il, filled, dminl, D, desp, p.radius, ws, wc), "refined")
    r = _pipe(Il, Ir, D, dminl, speckle=_p(30, 1.0), subpixel="parabola").results()
    z, c0, lo, hi, _ = subpix_ref.winners(plain["aggl"])
    _, subf = subpix_ref.maps(subpix_ref.MODES["parabola"], z, c0, lo, hi, plain["dmapl"], desp, filled, dminl)
    _eq(r["subpix_filled"], subf, "sub_filled")
    _eq(r["despeckled"], desp, "despeckled")


def test_pipeline_rejects_other_values_and_the_sharded_driver_refuses():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError):
        PairPipeline(64, 8, 4, speckle="on")
    with pytest.raises(ValueError):
        ShardedPair(64, 8, 4, speckle=True)


def test_context(pairs):
    Il, Ir, D, dminl, want, plain = pairs["tsukuba"]
    L = smx.lib()
    h, w = Il.shape
    n = w * h
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), w, h, D, C.byref(ctx)))
    try:
        bufs = {k: np.empty(n, np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        desp = np.empty(n, np.float32)
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0, C.byref(out)))
        assert L.smx_ctx_speckle_map(ctx, desp.ctypes.data) == -1              # that pair ran without it
        assert L.smx_ctx_set_speckle(ctx, C.byref(_p(-1, 1.0))) == -1
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_p(200, 1.0))))
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0, C.byref(out)))
        _lib.check(L.smx_ctx_speckle_map(ctx, desp.ctypes.data))
        r = _pipe(Il, Ir, D, dminl, speckle=True).results()
        _eq(desp.reshape(h, w), r["despeckled"], "ctx despeckled")
        _eq(bufs["filled"].reshape(h, w), r["filled"], "ctx filled")
        _eq(bufs["occlusion"].reshape(h, w), want["occlusion"], "ctx occlusion")
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0) == -1
        _lib.check(L.smx_ctx_set_speckle(ctx, None))
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0, C.byref(out)))
        _eq(bufs["filled"].reshape(h, w), want["filled"], "filled with the mode off again")
        assert L.smx_ctx_speckle_map(ctx, desp.ctypes.data) == -1
    finally:
        L.smx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# smx_main --speckle
# ---------------------------------------------------------------------------------------------
INDEPENDENT = ["image_left", "image_right", "image_mean_left", "image_mean_right", "best_costl", "best_costr",
               "cost_lminus15", "cost_rminus15", "occlu_mapl", "disparity_mapl", "disparity_mapr"]


@pytest.mark.parametrize("flags", [["--fused"], ["--host-compare"]])
def test_main_speckle(binary, tsukuba_oracle, orc, tmp_path, flags):
    PIL = pytest.importorskip("PIL.Image")
    runs = {}
    for name, extra in (("off", []), ("on", ["--speckle", "200,1"])):
        d = tmp_path / name
        (d / "data").mkdir(parents=True)
        for f in ("tsukuba0", "tsukuba1"):
            (d / "data" / (f + ".png")).write_bytes(open(os.path.join(ROOT, "tests", "golden", "tsukuba", f + ".png"), "rb").read())
        r = subprocess.run([binary] + flags + extra, cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "error at element" not in r.stdout
        runs[name] = d / "data"
        if extra and "--host-compare" in flags:
            assert "Speckle filter ok!" in r.stdout, r.stdout
    desp = ref.speckle_filter(tsukuba_oracle["occlusion"], -15, -115, 200, 1.0)
    _eq(np.asarray(PIL.open(runs["on"] / "occlu_mapl_despeckled.png")), smx.write_mat(desp), "occlu_mapl_despeckled.png")
    _eq(np.asarray(PIL.open(runs["on"] / "occlu_mapl_filled.png")), smx.write_mat(orc.fill_occlusion(desp, -15)),
        "occlu_mapl_filled.png")
    assert not (runs["off"] / "occlu_mapl_despeckled.png").exists()
    for name in INDEPENDENT:
        assert (runs["on"] / (name + ".png")).read_bytes() == (runs["off"] / (name + ".png")).read_bytes(), name
    golden = open(os.path.join(ROOT, "tests", "golden", "tsukuba", "occlu_mapl_filled.png"), "rb").read()
    assert (runs["off"] / "occlu_mapl_filled.png").read_bytes() == golden


def test_main_rejects_bad_speckle_options(binary, tmp_path):
    for bad in (["--speckle", "x"], ["--speckle", "-3"], ["--speckle", "5,-1"], ["--speckle", "5", "--pipeline"]):
        r = subprocess.run([binary] + bad, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--speckle" in r.stderr, bad
