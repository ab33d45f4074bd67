"""Semi-global matching on the GPU (smx_dev_sgm_wta_pair, smx_sgm_aggregate, PairPipeline(aggregation="sgm"), the context
entry), bit for bit against the numpy reference of tests/sgm_ref.py.  Every device call hands its buffers over inside
guard bands (tests/guarded.py) with the workspace poisoned and off its alignment, so each case checks the memory contract too.

Run on the GPU box:  python -m pytest tests -m gpu -q -k sgm
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import census_ref
import sgm_ref as ref
import speckle_ref
import subpix_ref
import wmf_ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 40, 9), (40, 5, 9), (65, 3, 63), (64, 4, 64), (63, 5, 65), (129, 70, 70),
          (130, 9, 192), (33, 6, 256)]
PENALTIES = [(10, 120), (0, 0), (7, 7), (4095, 4095)]


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


def _p(p1=10, p2=120, paths=8):
    p = _lib.SgmParams()
    p.p1, p.p2, p.paths = p1, p2, paths
    return p


class Call:
    """The buffers of one smx_dev_sgm_wta_pair call, every one guarded; cost_l / cost_r: (D, h, w) float32 or None."""

    def __init__(self, cost_l, cost_r, misalign=13, slots=None):
        self.costs = (cost_l, cost_r)
        D, h, w = (cost_l if cost_l is not None else cost_r).shape
        self.D, self.h, self.w, self.n = D, h, w, w * h
        self.nviews = (cost_l is not None) + (cost_r is not None)
        slots = self.nviews if slots is None else slots          # views the output buffers have room for
        n = self.n
        self.inp = [None if c is None else Guarded(c.nbytes, np.float32, c.shape, plane=n).load(c) for c in self.costs]
        self.keys = Guarded(slots * n * 8, np.int64, (slots, h, w), plane=n)
        self.agg = Guarded(slots * D * n * 4, np.float32, (slots, D, h, w), plane=n)
        self.nbr = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.ws_bytes = smx.lib().smx_sgm_workspace_bytes(w, h, D, self.nviews)
        assert self.ws_bytes > 0
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)
        self.ws.view.fill_(0xC3)                                  # poison: the call may rely on nothing in here

    def run(self, p, ws_bytes=None, agg=True, nbr=True):
        import torch
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda g: None if g is None else g.ptr
        return smx.lib().smx_dev_sgm_wta_pair(C.byref(p), ptr(self.inp[0]), ptr(self.inp[1]), self.w, self.h, self.D,
                                               self.keys.ptr, self.agg.ptr if agg else None, self.nbr.ptr if nbr else None,
                                               self.ws.ptr, self.ws_bytes if ws_bytes is None else ws_bytes, st)

    def check_memory(self):
        for g, name in ((self.keys, "d_keys"), (self.agg, "d_agg"), (self.nbr, "d_nbr"), (self.ws, "d_ws")):
            g.check(name)
        for g in self.inp:
            if g is not None:
                g.check_unchanged("d_cost")

    def check_against(self, p, label=""):
        """Run, then every output of every view equals the reference's, and nothing else was touched."""
        _lib.check(self.run(p))
        self.check_memory()
        keys, agg, nbr = self.keys.numpy(), self.agg.numpy(), self.nbr.numpy()
        slot = 0
        for c in self.costs:
            if c is None:
                continue
            want = ref.outputs(c, p.p1, p.p2, p.paths)
            _eq(agg[slot], want["agg"], f"{label} agg[{slot}]")
            _eq(keys[slot], want["keys"], f"{label} keys[{slot}]")
            _eq(nbr[slot], want["nbr"], f"{label} nbr[{slot}]")
            slot += 1


def _costs(seed, D, h, w, hi):
    return np.random.default_rng(seed).integers(0, hi + 1, (D, h, w)).astype(np.float32)


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("w,h,D", SHAPES)
def test_against_the_reference(w, h, D, paths):
    for hi in (62, 255):
        call = Call(_costs(w * 1000 + D + hi, D, h, w, hi), _costs(h * 1000 + D + hi + 1, D, h, w, hi))
        for p1, p2 in PENALTIES:
            call.check_against(_p(p1, p2, paths), f"{w}x{h}x{D} costs 0..{hi} p {p1},{p2}")


@pytest.mark.parametrize("paths", [4, 8])
def test_tie_rule(paths):
    w, h, D = 37, 6, 67
    const = np.full((D, h, w), 23, np.float32)
    rng = np.random.default_rng(5)
    # exactly two minima of the cost per pixel, and p1 = p2 = 0 so that S = paths * C keeps them both
    two = rng.integers(10, 200, (D, h, w)).astype(np.float32)
    za = rng.integers(0, D, (h, w))
    zb = (za + rng.integers(1, D, (h, w))) % D
    np.put_along_axis(two, za[None], 3, axis=0)
    np.put_along_axis(two, zb[None], 3, axis=0)
    call = Call(const, two)
    call.check_against(_p(10, 120, paths), "tie, default penalties")
    call.check_against(_p(0, 0, paths), "tie, no penalties")
    keys = call.keys.numpy()
    assert (keys[0] == smx.lib().smx_pack_key(float(paths * 23), D - 1)).all()          # constant: the LAST slice
    assert ((0xFFFFFFFF - (keys[1] & 0xFFFFFFFF)) == np.maximum(za, zb)).all()           # two minima: the later one


def test_special_values_go_through_the_clamp():
    w, h, D = 21, 5, 10
    specials = np.array([-1, -0.0, 0.0, 0.5, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40],
                        np.float32)
    rng = np.random.default_rng(9)
    cost = specials[rng.integers(0, specials.size, (D, h, w))]
    odd_nan = np.array([0xFFC00001, 0x7F800001], np.uint32).view(np.float32)         # a negative NaN, a signalling one
    cost[0, 0, :2] = odd_nan
    Call(cost, cost[:, ::-1].copy()).check_against(_p(), "special values")


@pytest.mark.parametrize("left", [True, False])
def test_one_view_forms_leave_the_other_view_alone(left):
    w, h, D = 19, 6, 66
    cost = _costs(11, D, h, w, 255)
    call = Call(cost if left else None, None if left else cost, slots=2)
    call.check_against(_p(), "one view")
    for g, name in ((call.keys, "keys"), (call.agg, "agg"), (call.nbr, "nbr")):
        tail = g.bytes[g.nbytes // 2:]
        assert bool((tail == g.fill).all()), f"{name}: the second view's half was written by a one-view call"


@pytest.mark.parametrize("misalign", [0, 1, 255])
def test_workspace_alignment_and_optional_outputs(misalign):
    w, h, D = 70, 9, 130
    cl, cr = _costs(21, D, h, w, 62), _costs(22, D, h, w, 62)
    Call(cl, cr, misalign=misalign).check_against(_p(), f"misalign {misalign}")
    call = Call(cl, cr, misalign=misalign)
    _lib.check(call.run(_p(), agg=False, nbr=False))
    call.check_memory()
    call.agg.check_untouched("d_agg (not requested)")
    call.nbr.check_untouched("d_nbr (not requested)")
    _eq(call.keys.numpy()[1], ref.outputs(cr)["keys"], "keys alone")


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    call = Call(_costs(31, 9, 5, 17, 62), _costs(32, 9, 5, 17, 62))
    call.ws.view.fill_(call.ws.fill)
    assert call.run(_p(), ws_bytes=call.ws_bytes - 1) == -3
    assert b"workspace" in smx.lib().smx_last_error()
    for g, name in ((call.keys, "d_keys"), (call.agg, "d_agg"), (call.nbr, "d_nbr"), (call.ws, "d_ws")):
        g.check_untouched(name)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    import torch
    w, h, D = 129, 70, 70
    call = Call(_costs(41, D, h, w, 62), _costs(42, D, h, w, 255))
    p = _p()
    _lib.check(call.run(p))
    first = [g.numpy().copy() for g in (call.keys, call.agg, call.nbr)]
    call.ws.view.fill_(0x11)
    _lib.check(call.run(p))
    for a, g, name in zip(first, (call.keys, call.agg, call.nbr), ("keys", "agg", "nbr")):
        _eq(g.numpy(), a, "second run " + name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.check(call.run(p))               # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(call.run(p))
    for g in (call.keys, call.agg, call.nbr):
        g.view.zero_()
    call.ws.view.fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, g, name in zip(first, (call.keys, call.agg, call.nbr), ("keys", "agg", "nbr")):
        _eq(g.numpy(), a, "graph replay " + name)
    call.check_memory()


def test_host_pointer_entry():
    w, h, D = 45, 11, 20
    cost = _costs(51, D, h, w, 62)
    p = _p(7, 50, 4)
    agg, best, disp = smx.sgm_aggregate(cost, dmin=-19, params=p)
    want = ref.outputs(cost, 7, 50, 4)
    _eq(agg, want["agg"], "agg")
    _eq(best, want["best"], "best")
    _eq(disp, (want["z"] - 19).astype(np.float32), "disp_map")
    assert smx.sgm_aggregate(cost, want_agg=False)[0] is None


# ---------------------------------------------------------------------------------------------
# the pipeline and the context
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL = 129, 70, 70, -69
SPK = (30, 1.0)


@pytest.fixture(scope="module")
def scene(orc):
    """The synthetic pair and the whole chain in numpy: census_ref -> sgm_ref -> the references of the later stages."""
    Il, Ir = synth.gen_pair(W, H, D, 4711)
    sl = ref.outputs(census_ref.census_cost(Il, Ir, D, DMINL))
    sr = ref.outputs(census_ref.census_cost(Ir, Il, D, 0))
    r = {"aggl": sl["agg"], "aggr": sr["agg"], "bestl": sl["best"], "bestr": sr["best"]}
    r["dmapl"] = (DMINL + sl["z"]).astype(np.float32)
    r["dmapr"] = sr["z"].astype(np.float32)
    r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], DMINL - 100)
    r["despeckled"] = speckle_ref.speckle_filter(r["occlusion"], DMINL, DMINL - 100, *SPK)
    r["filled"] = orc.fill_occlusion(r["despeckled"], DMINL)
    mode = subpix_ref.MODES["parabola"]
    r["subpixl"], r["subpix_filled"] = subpix_ref.maps(mode, sl["z"], sl["best"], sl["nbr"][0], sl["nbr"][1], r["dmapl"],
                                                       r["despeckled"], r["filled"], DMINL)
    r["subpixr"], _ = subpix_ref.maps(mode, sr["z"], sr["best"], sr["nbr"][0], sr["nbr"][1], r["dmapr"])
    wp = smx.default_wmf_params()
    ws, wc = smx.wmf_weights(wp)
    r["refined"] = wmf_ref.weighted_median(Il, r["filled"], DMINL, D, r["despeckled"], wp.radius, ws, wc)
    return Il, Ir, r


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


def _pipe(Il, Ir, **kw):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(W, H, D, dminl=DMINL, **kw)
    pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
    return pipe


def test_pipeline(scene):
    Il, Ir, want = scene
    pipe = _pipe(Il, Ir, cost="census", aggregation="sgm", subpixel="parabola", speckle=_spk(), wmf="occluded", want_agg=True)
    assert pipe.sgm_ws is not None and pipe.sgm_cost is not None and pipe.sgm_params.paths == 8
    got = pipe.results()
    for k in ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "despeckled", "filled", "subpixl", "subpixr",
              "subpix_filled", "refined"):
        _eq(got[k], want[k], k)
    assert np.any(want["despeckled"] != want["occlusion"]) and np.any(want["refined"] != want["filled"])


def test_pipeline_refuses_what_sgm_cannot_do():
    from stereo_matching_cuda_amd.device import PairPipeline
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, aggregation="sgm", s_begin=0, s_end=D // 2)
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, aggregation="sgm", max_ws_bytes=1 << 20)
    with pytest.raises(ValueError):
        PairPipeline(W, H, 257, aggregation="sgm")


def test_reference_cost_goes_through_the_clamp(scene, orc):
    Il, Ir, _ = scene
    got = _pipe(Il, Ir, aggregation="sgm", sgm_params=_p(5, 40, 4), want_agg=True).results()
    for k, (a, b, dmin) in (("aggl", (Il, Ir, DMINL)), ("aggr", (Ir, Il, 0))):
        _eq(got[k], ref.outputs(orc.cost_volume(a, b, D, dmin), 5, 40, 4)["agg"], k)


def test_aggregation_none_changes_nothing(scene):
    Il, Ir, _ = scene
    a = _pipe(Il, Ir, aggregation=None)
    assert a.sgm_ws is None and a.sgm_cost is None and a.sgm_params is None and a.aggregation is None
    b = _pipe(Il, Ir)
    ra, rb = a.results(), b.results()
    assert ra.keys() == rb.keys()
    for k in ra:
        _eq(ra[k], rb[k], k)
    assert a.ws_bytes == b.ws_bytes


def test_context(scene):
    Il, Ir, want = scene
    L = smx.lib()
    n = W * H
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), W, H, D, C.byref(ctx)))
    try:
        assert L.smx_ctx_set_aggregation(ctx, 2, None) == -1
        assert L.smx_ctx_set_aggregation(ctx, 1, C.byref(_p(11, 10, 8))) == -1
        _lib.check(L.smx_ctx_set_cost(ctx, 1, None))
        _lib.check(L.smx_ctx_set_aggregation(ctx, 1, None))
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk())))
        bufs = {k: np.empty(n, np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
        bufs["agg_l"], bufs["agg_r"] = np.empty(D * n, np.float32), np.empty(D * n, np.float32)
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, 0, C.byref(out)))
        for k, name in (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"),
                        ("occlusion", "occlusion"), ("filled", "filled"), ("agg_l", "aggl"), ("agg_r", "aggr")):
            _eq(bufs[k].reshape(want[name].shape), want[name], "ctx " + name)
        sub = [np.empty((H, W), np.float32) for _ in range(3)]
        _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
        for s, name in zip(sub, ("subpixl", "subpixr", "subpix_filled")):
            _eq(s, want[name], "ctx " + name)
        desp = np.empty((H, W), np.float32)
        _lib.check(L.smx_ctx_speckle_map(ctx, desp.ctypes.data))
        _eq(desp, want["despeckled"], "ctx despeckled")
        mean = np.empty(n, np.uint8)
        out.mean_l = mean.ctypes.data
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, 0, C.byref(out)) == -1
        assert b"mean" in L.smx_last_error()
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, 0) == -1
    finally:
        L.smx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# usefulness: a textureless patch wider than the guided filter's window
# ---------------------------------------------------------------------------------------------
def _patch_scene(seed=3, w=129, h=70, size_d=16, split=40, d_left=9, d_right=3, rows=(20, 50), cols=(60, 100)):
    """Two fronto-parallel random textures (disparity 9 left of column 40, 3 right of it) and, inside the second one, a
    constant patch of 40 x 30 pixels: wider and taller than the 19 x 19 window.  -> left, right, the true left labels."""
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 256, (h, w + size_d)).astype(np.uint8)
    truth = np.where(np.arange(w) < split, d_left, d_right)[None, :].repeat(h, 0)
    left = np.take_along_axis(R, np.arange(w)[None, :] - truth + size_d, axis=1)
    left[rows[0]:rows[1], cols[0]:cols[1]] = 128
    R[rows[0]:rows[1], cols[0] - d_right + size_d:cols[1] - d_right + size_d] = 128
    return np.ascontiguousarray(left), np.ascontiguousarray(R[:, size_d:size_d + w]), -truth.astype(np.float32)


def test_sgm_bridges_a_textureless_patch_that_the_window_filter_does_not(orc):
    """Exact by construction: on the committed scene (seed 3) the references alone -- census_ref -> the oracle's guided
    filter or sgm_ref -> the oracle's LR check and fill -- give 29 wrong pixels (|d - truth| > 1) for the guided filter and 0
    for SGM, and the pipelines equal their references bit for bit."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    size_d, dminl = 16, -15
    Il, Ir, truth = _patch_scene()
    h, w = Il.shape
    cl, cr = census_ref.census_cost(Il, Ir, size_d, dminl), census_ref.census_cost(Ir, Il, size_d, 0)
    finish = lambda dl, dr: orc.fill_occlusion(orc.detect_occlusion(dl, dr, dminl - 100), dminl)
    want = {"guided": finish(orc.guided_filter(Il, cl, dminl)[1], orc.guided_filter(Ir, cr, 0)[1]),
            "sgm": finish((dminl + ref.outputs(cl)["z"]).astype(np.float32), ref.outputs(cr)["z"].astype(np.float32))}
    wrong = {}
    for name, kw in (("guided", {}), ("sgm", {"aggregation": "sgm"})):
        pipe = PairPipeline(w, h, size_d, dminl=dminl, cost="census", **kw)
        pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
        filled = pipe.results()["filled"]
        _eq(filled, want[name], name + " filled")
        wrong[name] = int((np.abs(filled - truth) > 1).sum())
    print("wrong pixels:", wrong)
    assert wrong["sgm"] < wrong["guided"], wrong
