"""The weighted-median refinement on the GPU (smx_weighted_median / smx_dev_weighted_median, PairPipeline(wmf=...),
smx_main --wmf), bit-exact against the numpy reference of tests/wmf_ref.py with the library's own weight tables.

Run on the GPU box:  python -m pytest tests -m gpu -q -k wmf
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import wmf_ref
from main_harness import binary  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eq(a, b, name=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        both_nan = np.isnan(a) & np.isnan(b)       # NaN payload / sign is not part of the contract
        a, b = a.view(np.uint32), b.view(np.uint32)
        a = np.where(both_nan, 0, a)
        b = np.where(both_nan, 0, b)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _params(radius=9, sigma_s=9.0, sigma_c=25.5):
    p = _lib.WmfParams()
    p.radius, p.sigma_s, p.sigma_c = radius, sigma_s, sigma_c
    return p


def _ref(guide, disp, dmin, size_d, select=None, params=None):
    p = params if params is not None else smx.default_wmf_params()
    ws, wc = smx.wmf_weights(p)
    return wmf_ref.weighted_median(guide, disp, dmin, size_d, select, p.radius, ws, wc)


def _check(guide, disp, dmin, size_d, select=None, params=None, name=""):
    got = smx.weighted_median(guide, disp, dmin, size_d, select=select, params=params)
    _eq(got, _ref(guide, disp, dmin, size_d, select, params), name)
    return got


def _messy(rng, h, w, dmin, size_d):
    d = (dmin + rng.integers(0, size_d, size=(h, w))).astype(np.float32)
    m = rng.random((h, w))
    d[m < 0.04] = np.nan
    d[(m >= 0.04) & (m < 0.06)] = np.inf
    d[(m >= 0.06) & (m < 0.08)] = -np.inf
    d[(m >= 0.08) & (m < 0.12)] = dmin - 100
    d[(m >= 0.12) & (m < 0.15)] += 0.25
    d[(m >= 0.15) & (m < 0.17)] = dmin + size_d
    d[(m >= 0.17) & (m < 0.19)] = -0.0
    return d


# ---------------------------------------------------------------------------------------------
# Tsukuba: the oracle's filled / occlusion maps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["occluded", "all"])
def test_tsukuba(tsukuba_oracle, tsukuba_gray, mode):
    filled, occ = tsukuba_oracle["filled"], tsukuba_oracle["occlusion"]
    sel = occ if mode == "occluded" else None
    got = _check(tsukuba_gray[0], filled, -15, 16, sel, name=f"tsukuba {mode}")
    if mode == "occluded":
        picked = wmf_ref.selected(occ, -15, occ.shape)
        assert int(picked.sum()) == 10605
        _eq(got[~picked], filled[~picked], "not selected")
        assert np.any(got[picked] != filled[picked])      # the refinement changed something


# ---------------------------------------------------------------------------------------------
# shapes, label ranges, inputs, parameters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,radius", [(1, 1, 9), (1, 300, 9), (200, 1, 9), (3, 5, 15), (37, 70, 9), (9, 130, 4),
                                        (2, 20000, 9), (65, 64, 15)])
def test_shapes(h, w, radius):
    rng = np.random.default_rng(h * 7 + w)
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = _messy(rng, h, w, -10, 24)
    p = _params(radius)
    _check(g, d, -10, 24, None, p, f"{h}x{w} all")
    sel = np.where(rng.random((h, w)) < 0.3, np.float32(-110), np.float32(-3)).astype(np.float32)
    _check(g, d, -10, 24, sel, p, f"{h}x{w} random selection")


@pytest.mark.parametrize("dmin,size_d", [(0, 1), (-7, 1), (-15, 16), (-191, 192), (5, 17), (0, 63), (-64, 65),
                                         (-2000, 4096), (100, 4096), (-4095, 4096)])
def test_label_ranges(dmin, size_d):
    rng = np.random.default_rng(size_d + 7)
    h, w = 40, 100
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    # labels on both sides of every bucket boundary of the two-level histogram (buckets of 2^shift labels,
    # 4^shift >= size_d), on the range ends, and anywhere
    shift = 0
    while 4 ** shift < size_d:
        shift += 1
    edges = np.arange(0, size_d + 1, 1 << shift)
    near = np.unique(np.clip(np.concatenate([edges - 1, edges, [0, size_d - 1]]), 0, size_d - 1))
    k = np.where(rng.random((h, w)) < 0.7, rng.choice(near, size=(h, w)), rng.integers(0, size_d, size=(h, w)))
    d = (dmin + k).astype(np.float32)
    _check(g, d, dmin, size_d, None, None, f"[{dmin}, {dmin + size_d})")
    # one window straddling a boundary: two labels either side of it, weights that put the median on each side
    inner = edges[1:-1]
    for e in inner[::max(1, len(inner) // 5)]:
        d2 = np.where(np.arange(w)[None, :] < w // 2, dmin + e - 1, dmin + e).astype(np.float32).repeat(h, 0)
        _check(g, d2, dmin, size_d, None, _params(4), f"edge {e}")


def test_inputs_that_count_for_nothing_or_are_copied():
    rng = np.random.default_rng(11)
    h, w, dmin, size_d = 50, 90, -15, 16
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = _messy(rng, h, w, dmin, size_d)
    d[10:20, 10:40] = np.nan                  # windows with nothing that counts: the input is copied
    d[30:45, 50:85] = dmin - 100
    none = np.full((h, w), np.float32(dmin), np.float32)
    sel_all = np.full((h, w), np.float32(dmin - 100), np.float32)
    sel_odd = rng.choice(np.array([np.nan, np.inf, -np.inf, dmin - 0.5, dmin - 1, dmin, -0.0, -1e30, 1e30],
                                  np.float32), size=(h, w))
    for name, sel in (("all", None), ("select every pixel", sel_all), ("select none", none), ("odd selects", sel_odd)):
        got = _check(g, d, dmin, size_d, sel, None, name)
        if name == "select none":
            _eq(got, d, "copied bit for bit")
    _eq(smx.weighted_median(g, d, dmin, size_d, sel_all), smx.weighted_median(g, d, dmin, size_d), "all == NULL")


@pytest.mark.parametrize("radius,sigma_s,sigma_c", [(1, 9.0, 25.5), (9, 9.0, 25.5), (15, 9.0, 25.5),
                                                     (15, 1e9, 1e9), (9, 0.05, 0.3), (15, 0.4, 0.2), (5, 2.0, 1e-3)])
def test_parameters(radius, sigma_s, sigma_c):
    rng = np.random.default_rng(radius)
    h, w, dmin, size_d = 45, 77, -30, 40
    g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    d = _messy(rng, h, w, dmin, size_d)
    p = _params(radius, sigma_s, sigma_c)
    got = _check(g, d, dmin, size_d, None, p, "params")
    if sigma_c < 0.5:          # range weights 0 beyond t = 0: pixels whose window has no equal gray keep their input
        ws, wc = smx.wmf_weights(p)
        assert wc[1] == 0
        assert np.any(np.isnan(got)) or np.any(got == d)


# ---------------------------------------------------------------------------------------------
# the device entry: streams, graph capture, host entry == device entry, and the pipeline
# ---------------------------------------------------------------------------------------------
def _dev_call(t_g, t_d, t_s, t_o, dmin, size_d, stream, params=None):
    import torch
    h, w = t_d.shape
    p = params if params is not None else smx.default_wmf_params()
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    smx.check(smx.lib().smx_dev_weighted_median(C.byref(p), dp(t_g), dp(t_d), dp(t_s), dp(t_o), w, h, dmin, size_d,
                                                C.c_void_p(stream.cuda_stream)))


def test_device_entry_on_a_side_stream_and_in_a_graph(tsukuba_oracle, tsukuba_gray):
    import torch
    filled, occ = tsukuba_oracle["filled"], tsukuba_oracle["occlusion"]
    t_g = torch.from_numpy(tsukuba_gray[0]).cuda()
    t_d = torch.from_numpy(filled).cuda()
    t_s = torch.from_numpy(occ).cuda()
    for sel, t_sel in ((occ, t_s), (None, None)):
        want = _ref(tsukuba_gray[0], filled, -15, 16, sel)
        _eq(smx.weighted_median(tsukuba_gray[0], filled, -15, 16, sel), want, "host entry")
        side = torch.cuda.Stream()
        t_o = torch.full_like(t_d, -1.0)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _dev_call(t_g, t_d, t_sel, t_o, -15, 16, side)
        side.synchronize()
        _eq(t_o.cpu().numpy(), want, "side stream")
        # a single-stream capture: the call is one kernel launch, no allocation, no synchronisation
        t_o2 = torch.full_like(t_d, -1.0)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                _dev_call(t_g, t_d, t_sel, t_o2, -15, 16, s)
        torch.cuda.synchronize()
        t_o2.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        _eq(t_o2.cpu().numpy(), want, "graph replay")


def _kitti_pipeline(wmf):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    w, h, D = synth.SHAPES["kitti"]
    Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS["kitti"])
    pipe = PairPipeline(w, h, D, wmf=wmf)
    pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
    return Il, pipe


@pytest.fixture(scope="module")
def kitti_plain():
    Il, pipe = _kitti_pipeline(None)
    assert pipe.refined is None
    r = pipe.results()
    assert "refined" not in r
    return Il, r


@pytest.mark.parametrize("mode", ["occluded", "all"])
def test_kitti_pipeline(kitti_plain, mode):
    Il, plain = kitti_plain
    _, pipe = _kitti_pipeline(mode)
    r = pipe.results()
    for k, v in plain.items():
        _eq(r[k], v, k)
    D = synth.SHAPES["kitti"][2]
    sel = r["occlusion"] if mode == "occluded" else None
    want = _ref(Il, r["filled"], -(D - 1), D, sel)       # the whole image
    _eq(r["refined"], want, f"refined {mode}")


def test_pipeline_rejects_unknown_modes():
    from stereo_matching_cuda_amd.device import PairPipeline
    with pytest.raises(ValueError):
        PairPipeline(64, 8, 4, wmf="median")


# ---------------------------------------------------------------------------------------------
# smx_main --wmf
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


@pytest.mark.parametrize("flags", [["--fused", "--wmf", "occluded"], ["--wmf", "all", "--host-compare"]])
def test_main_wmf(binary, tsukuba_oracle, tsukuba_gray, tmp_path, flags):
    PIL = pytest.importorskip("PIL.Image")
    data = _stage(tmp_path)
    pfm = tmp_path / "d.pfm"
    r = subprocess.run([binary] + flags + ["--pfm", str(pfm)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "error at element" not in r.stdout
    if "--host-compare" in flags:
        assert "Weighted median ok!" in r.stdout, r.stdout
    mode = flags[flags.index("--wmf") + 1]
    sel = tsukuba_oracle["occlusion"] if mode == "occluded" else None
    want = _ref(tsukuba_gray[0], tsukuba_oracle["filled"], -15, 16, sel)
    _eq(np.asarray(PIL.open(data / "occlu_mapl_wmf.png")), smx.write_mat(want), "occlu_mapl_wmf.png")
    raw = pfm.read_bytes()
    rest = raw.split(b"\n", 3)[3]
    d = np.frombuffer(rest, "<f4").reshape(288, 384)[::-1]
    _eq(np.ascontiguousarray(d), -want, "pfm")
    for name in OUTPUTS:        # the reference's 12 files are untouched by the refinement
        ref = open(os.path.join(ROOT, "tests", "golden", "tsukuba", name + ".png"), "rb").read()
        assert (data / (name + ".png")).read_bytes() == ref, name


def test_main_rejects_a_bad_wmf_mode(binary, tmp_path):
    r = subprocess.run([binary, "--wmf", "median"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--wmf" in r.stderr
