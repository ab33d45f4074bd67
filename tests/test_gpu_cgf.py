"""The colour-guided filter aggregation on the GPU (smx_dev_cgf_wta_pair, smx_colour_guided_filter), bit for bit against the
numpy reference of tests/cgf_ref.py.  Every device call hands its buffers over inside guard bands (tests/guarded.py) with the
workspace poisoned and off its alignment, so each case checks the memory contract too.

Run on the GPU box:  python -m pytest tests -m gpu -q -k cgf
"""
import ctypes as C
import functools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import census_ref
import cgf_ref as ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

# 31 / 32 / 33: one column either side of the row scan's tile of 32 columns; 64 / 65 rows: either side of its band
SHAPES = [(1, 1, 1), (2, 1, 3), (1, 7, 2), (19, 40, 5), (65, 3, 4), (64, 4, 4), (63, 5, 4), (31, 64, 2), (32, 65, 2), (33, 6, 2),
          (129, 70, 9), (210, 150, 3)]
RADII = (0, 1, 9, 12)
EPS = (6.5025, 0.5)
COSTS = ("floats", "synth", "census")
GUIDES = ("random", "flat", "isoluminant")


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


def _p(radius=9, eps=6.5025):
    p = smx.default_params()
    p.radius, p.eps = radius, eps
    return p


@functools.lru_cache(maxsize=None)
def _costs(kind, w, h, D, view):
    """(D, h, w) float32, read-only"""
    if kind == "floats":
        c = (np.random.default_rng(1000 * w + 10 * h + D + view).random((D, h, w)) * 8).astype(np.float32)
    else:
        import oracle
        oracle.build()
        ww = max(w, 2)                              # (the reference's x derivative needs two columns)
        Il, Ir = synth.gen_pair(ww, h, D, 77 + w + h)
        a, b, dmin = (Il, Ir, 1 - D) if view == 0 else (Ir, Il, 0)
        c = oracle.cost_volume(a, b, D, dmin) if kind == "synth" else census_ref.census_cost(a, b, D, dmin)
        c = np.ascontiguousarray(c[:, :, :w], np.float32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _guide(kind, w, h, view, channels=3):
    rng = np.random.default_rng(500 * w + h + view)
    if kind == "random":
        g = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    elif kind == "flat":
        g = np.empty((h, w, channels), np.uint8)
        g[:] = rng.integers(0, 256, channels, dtype=np.uint8)
    else:
        import oracle
        oracle.build()
        ca, cb, _ = ref.isoluminant_pair(oracle.gray)
        g = np.full((h, w, channels), 255, np.uint8)
        g[:, :, :3] = np.where((rng.random((h, w)) < 0.5)[:, :, None], ca, cb)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=32)
def _want(gkind, ckind, w, h, D, view, radius, eps, channels=3):
    q = ref.aggregate(_guide(gkind, w, h, view, channels), _costs(ckind, w, h, D, view), radius, eps)
    q.setflags(write=False)
    return q


class Call:
    """The buffers of smx_dev_cgf_wta_pair calls on one pair, every one guarded.  rgb_*: (h, w, ch) uint8 or None,
    cost_*: (D, h, w) float32 or None; a call covers slices [s0, s1) of them."""

    def __init__(self, rgb_l, cost_l, rgb_r, cost_r, ws_slices=None, misalign=13, slots=None):
        self.rgbs, self.costs = (rgb_l, rgb_r), (cost_l, cost_r)
        some = cost_l if cost_l is not None else cost_r
        D, h, w = some.shape
        self.D, self.h, self.w, self.n = D, h, w, w * h
        self.ch = (rgb_l if rgb_l is not None else rgb_r).shape[2]
        self.nviews = (cost_l is not None) + (cost_r is not None)
        slots = self.nviews if slots is None else slots
        n = self.n
        self.grgb = [None if g is None else Guarded(g.nbytes, np.uint8, g.shape, plane=n, misalign=3).load(g) for g in self.rgbs]
        self.gcost = [None if c is None else Guarded(c.nbytes, np.float32, c.shape, plane=n).load(c) for c in self.costs]
        self.keys = Guarded(slots * n * 8, np.int64, (slots, h, w), plane=n)
        self.agg = Guarded(slots * D * n * 4, np.float32, (slots, D, h, w), plane=n)
        self.nbr = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.uq = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.ws_bytes = smx.lib().smx_cgf_workspace_bytes(w, h, D if ws_slices is None else ws_slices, self.nviews)
        assert self.ws_bytes > 0
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)
        self.poison()
        self.init_keys()

    def poison(self, byte=0xC3):
        self.ws.view.fill_(byte)                    # the call may rely on nothing in here (0xC3C3C3C3 is a float of -391.5)

    def init_keys(self):
        self.keys.view.fill_(np.iinfo(np.int64).max)

    def run(self, p, s0=0, s1=None, ws_bytes=None, agg=True, nbr=True, uq=True):
        import torch
        s1 = self.D if s1 is None else s1
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda g: None if g is None else g.ptr
        off = lambda g, b: None if g is None else C.c_void_p(g.ptr.value + b)
        # d_cost / d_agg of a call start at its first slice
        return smx.lib().smx_dev_cgf_wta_pair(
            C.byref(p), ptr(self.grgb[0]), ptr(self.grgb[1]), self.ch, off(self.gcost[0], s0 * self.n * 4),
            off(self.gcost[1], s0 * self.n * 4), self.w, self.h, s0, s1, self.keys.ptr, self.agg.ptr if agg else None,
            self.nbr.ptr if nbr else None, self.uq.ptr if uq else None, self.ws.ptr,
            self.ws_bytes if ws_bytes is None else ws_bytes, st)

    def check_memory(self):
        for g, name in ((self.keys, "d_keys"), (self.agg, "d_agg"), (self.nbr, "d_nbr"), (self.uq, "d_uq"), (self.ws, "d_ws")):
            g.check(name)
        for g in self.grgb + self.gcost:
            if g is not None:
                g.check_unchanged("an input")

    def check_outputs(self, wants, label="", agg=True):
        """wants: the aggregated volume of every view of the call, in order"""
        self.check_memory()
        keys, got, nbr, uq = self.keys.numpy(), self.agg.numpy(), self.nbr.numpy(), self.uq.numpy()
        for slot, q in enumerate(wants):
            st = ref.states(q)
            if agg:
                _eq(got[slot], q, f"{label} agg[{slot}]")
            _eq(keys[slot], st["keys"], f"{label} keys[{slot}]")
            _eq(nbr[slot], st["nbr"], f"{label} nbr[{slot}]")
            _eq(uq[slot], st["uq"], f"{label} uq[{slot}]")


def _pair(gkind, ckind, w, h, D, **kw):
    return Call(_guide(gkind, w, h, 0), _costs(ckind, w, h, D, 0), _guide(gkind, w, h, 1), _costs(ckind, w, h, D, 1), **kw)


@pytest.mark.parametrize("ckind", COSTS)
@pytest.mark.parametrize("w,h,D", SHAPES)
def test_against_the_reference(w, h, D, ckind):
    for gkind in GUIDES:
        call = _pair(gkind, ckind, w, h, D)
        for radius in RADII:
            for eps in EPS:
                call.poison()
                call.init_keys()
                _lib.check(call.run(_p(radius, eps)))
                call.check_outputs([_want(gkind, ckind, w, h, D, v, radius, eps) for v in (0, 1)],
                                   f"{w}x{h}x{D} {ckind} {gkind} r{radius} eps{eps}")


@pytest.mark.parametrize("left", [True, False])
def test_one_view_forms_leave_the_other_view_alone(left):
    for (w, h, D), radius in (((19, 40, 5), 12), ((129, 70, 9), 9), ((33, 6, 2), 1)):
        v = 0 if left else 1
        g, c = _guide("random", w, h, v), _costs("floats", w, h, D, v)
        call = Call(g if left else None, c if left else None, None if left else g, None if left else c, slots=2)
        _lib.check(call.run(_p(radius)))
        call.check_outputs([_want("random", "floats", w, h, D, v, radius, 6.5025)], "one view")
        assert bool((call.keys.view[1] == np.iinfo(np.int64).max).all()), "keys: the second view's half was written"
        for buf, name in ((call.agg, "agg"), (call.nbr, "nbr"), (call.uq, "uq")):
            assert bool((buf.bytes[buf.nbytes // 2:] == buf.fill).all()), f"{name}: the second view's half was written by a one-view call"


def test_four_channels_and_optional_outputs():
    w, h, D = 65, 9, 3
    cl, cr = _costs("floats", w, h, D, 0), _costs("floats", w, h, D, 1)
    g3 = [_guide("random", w, h, v) for v in (0, 1)]
    g4 = [np.concatenate((g, np.full((h, w, 1), 7 + v, np.uint8)), axis=2) for v, g in enumerate(g3)]
    wants = [_want("random", "floats", w, h, D, v, 9, 6.5025) for v in (0, 1)]
    for misalign in (0, 1, 255):
        call = Call(g4[0], cl, g4[1], cr, misalign=misalign)
        _lib.check(call.run(_p()))
        call.check_outputs(wants, f"rgba, misalign {misalign}")
    call = Call(g3[0], cl, g3[1], cr)
    _lib.check(call.run(_p(), agg=False, nbr=False, uq=False))
    call.check_memory()
    for g, name in ((call.agg, "d_agg"), (call.nbr, "d_nbr"), (call.uq, "d_uq")):
        g.check_untouched(name + " (not requested)")
    for v in (0, 1):
        _eq(call.keys.numpy()[v], ref.states(wants[v])["keys"], "keys alone")


def test_special_costs_and_a_degenerate_inverse_propagate():
    """NaN / inf costs and det <= 0 (eps = 0 on a flat guide: 0 / 0) get no special treatment: the bits are the reference's,
    and a NaN never wins."""
    w, h, D = 40, 9, 4
    rng = np.random.default_rng(61)
    cost = (rng.random((D, h, w)) * 8).astype(np.float32)
    cost[1, 3, 5], cost[2, 0, 0], cost[0, 8, 39], cost[3, 4, 20] = np.nan, np.inf, -np.inf, -0.0
    for gkind, eps in (("random", 6.5025), ("flat", 0.0), ("isoluminant", 0.0)):
        g = _guide(gkind, w, h, 0)
        call = Call(g, cost, g, cost[::-1].copy())
        _lib.check(call.run(_p(2, eps)))
        with np.errstate(all="ignore"):
            call.check_outputs([ref.aggregate(g, cost, 2, eps), ref.aggregate(g, cost[::-1], 2, eps)], f"{gkind} eps {eps}")


# ---------------------------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------------------------
W, H, D = 129, 70, 9


@pytest.fixture(scope="module")
def wants():
    return [_want("random", "synth", W, H, D, v, 9, 6.5025) for v in (0, 1)]


@pytest.mark.parametrize("ws_slices", [1, 2, D])
def test_the_workspace_size_does_not_change_a_bit(wants, ws_slices):
    call = _pair("random", "synth", W, H, D, ws_slices=ws_slices)
    _lib.check(call.run(_p()))
    call.check_outputs(wants, f"workspace for {ws_slices} slices")


def test_max_slices_per_launch_does_not_change_a_bit(wants):
    call = _pair("random", "synth", W, H, D)
    L = smx.lib()
    try:
        for k in (1, 4):
            _lib.check(L.smx_set_max_slices_per_launch(k))
            call.poison()
            call.init_keys()
            _lib.check(call.run(_p()))
            call.check_outputs(wants, f"max slices per launch {k}")
    finally:
        L.smx_set_max_slices_per_launch(0)


@pytest.mark.parametrize("k", [1, 4, 8])
def test_two_calls_on_one_set_of_keys_carry_the_states_across(wants, k):
    call = _pair("random", "synth", W, H, D, ws_slices=3)
    _lib.check(call.run(_p(), 0, k))
    call.poison(0x3C)
    # (d_agg of a call starts at its first slice: the second call writes D - k slices per view from the front)
    first = call.agg.numpy().copy()
    _lib.check(call.run(_p(), k, D))
    call.check_outputs(wants, f"[0, {k}) then [{k}, {D})", agg=False)
    second = call.agg.numpy()
    # the layout of a call's d_agg is (views, s1 - s0, h, w) from the front of the buffer
    n = W * H
    for v in (0, 1):
        _eq(first.reshape(-1)[v * k * n:(v + 1) * k * n].reshape(k, H, W), wants[v][:k], f"agg of [0, {k}) view {v}")
        _eq(second.reshape(-1)[v * (D - k) * n:(v + 1) * (D - k) * n].reshape(D - k, H, W), wants[v][k:], f"agg of [{k}, {D}) view {v}")


def test_keys_accumulate_by_the_min(wants):
    """IN/OUT keys: a call over [k, D) on keys that hold a better winner of another shard keeps it."""
    call = _pair("random", "synth", W, H, D)
    best = smx.lib().smx_pack_key(-1.0, 2)
    call.keys.view.fill_(best)
    _lib.check(call.run(_p(), nbr=False, uq=False))
    assert bool((call.keys.view == best).all())
    call.check_memory()


# ---------------------------------------------------------------------------------------------
# runtime and memory behaviour
# ---------------------------------------------------------------------------------------------
def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    call = _pair("random", "floats", 19, 40, 5, ws_slices=1)
    call.ws.view.fill_(call.ws.fill)
    call.keys.bytes.fill_(call.keys.fill)
    assert call.run(_p(), ws_bytes=call.ws_bytes - 1) == -3
    assert b"workspace" in smx.lib().smx_last_error()
    for g, name in ((call.keys, "d_keys"), (call.agg, "d_agg"), (call.nbr, "d_nbr"), (call.uq, "d_uq"), (call.ws, "d_ws")):
        g.check_untouched(name)
    call.init_keys()
    call.poison()
    _lib.check(call.run(_p()))                       # ... and exactly that many bytes are enough
    call.check_outputs([_want("random", "floats", 19, 40, 5, v, 9, 6.5025) for v in (0, 1)], "smallest workspace")


def test_two_runs_and_a_graph_replay_give_the_same_bits(wants):
    import torch
    call = _pair("random", "synth", W, H, D, ws_slices=4)
    p = _p()
    outs = (call.keys, call.agg, call.nbr, call.uq)
    names = ("keys", "agg", "nbr", "uq")
    _lib.check(call.run(p))
    call.check_outputs(wants, "first run")
    first = [g.numpy().copy() for g in outs]
    call.poison(0x11)
    call.init_keys()
    _lib.check(call.run(p))
    for a, g, name in zip(first, outs, names):
        _eq(g.numpy(), a, "second run " + name)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call.init_keys()
        _lib.check(call.run(p))               # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(call.run(p))
    for _ in range(2):
        for g in outs[1:]:
            g.view.zero_()
        call.init_keys()
        call.poison(0x77)
        graph.replay()
        torch.cuda.synchronize()
        for a, g, name in zip(first, outs, names):
            _eq(g.numpy(), a, "graph replay " + name)
    call.check_memory()


def test_host_pointer_entry(orc):
    w, h, D = 45, 11, 6
    g, cost = _guide("random", w, h, 0), _costs("floats", w, h, D, 0)
    p = _p(3, 0.5)
    best, dmap = smx.init_wta(h, w)
    agg = smx.colour_guided_filter(g, cost, best, dmap, -5, want_agg=True, params=p)
    q = ref.aggregate(g, cost, 3, 0.5)
    st = ref.states(q)
    _eq(agg, q, "agg")
    _eq(best, st["best"], "filter_cost")
    _eq(dmap, (st["z"] - 5).astype(np.float32), "disp_map")
    # IN/OUT like the reference's: a pixel is updated iff filter_cost >= min q
    best2 = np.full((h, w), -1.0, np.float32)
    dmap2 = np.full((h, w), 3.0, np.float32)
    assert smx.colour_guided_filter(g, cost, best2, dmap2, -5, params=p) is None
    assert (best2 == -1).all() and (dmap2 == 3).all()


# ---------------------------------------------------------------------------------------------
# the reason for the feature
# ---------------------------------------------------------------------------------------------
def test_the_isoluminant_edge_on_the_gpu(orc):
    """Two slices: slice 0 is cheap left of x = 32, slice 1 right of it.  The colour guide keeps the step of the winner at
    x = 32; the gray guide has no edge there, and the aggregated costs next to the step are the double box blur."""
    rgb, p, _ = ref.isoluminant_scene(orc.gray)
    cost = np.concatenate((p, 1 - p)).astype(np.float32)                 # slice 0 wins left of the split, slice 1 right
    h, w = rgb.shape[:2]
    best, dmap = smx.init_wta(h, w)
    agg = smx.colour_guided_filter(rgb, cost, best, dmap, 0, want_agg=True)
    _eq(agg, ref.aggregate(rgb, cost), "agg")
    assert np.abs(agg[0] - cost[0])[:, 31:33].max() < 0.1
    assert (dmap[:, :32] == 0).all() and (dmap[:, 32:] == 1).all()
    gb, gd = smx.init_wta(h, w)
    _, gagg = smx.compute_guided_filter(orc.gray(rgb), cost, gb, gd, 0, want_agg=True)
    assert np.abs(gagg[0] - cost[0])[:, 31:33].min() > 0.3


# ---------------------------------------------------------------------------------------------
# the pipeline and the context
# ---------------------------------------------------------------------------------------------
PW, PH, PD, PDMINL = 129, 70, 16, -15
SPK = (30, 1.0)
RATIO = 0.15


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


def chain(orc, rgb_l, rgb_r, census):
    """The whole pair in numpy: gray -> cost (census: False the reference's, True census, "adcensus") -> cgf_ref -> the
    references of the later stages."""
    import adcensus_ref
    import speckle_ref
    import subpix_ref
    import uniq_ref
    import wmf_ref
    Il, Ir = orc.gray(rgb_l), orc.gray(rgb_r)
    cost = (lambda a, b, dmin: adcensus_ref.gray_cost(a, b, PD, dmin)) if census == "adcensus" else \
           (lambda a, b, dmin: census_ref.census_cost(a, b, PD, dmin)) if census else \
           (lambda a, b, dmin: orc.cost_volume(a, b, PD, dmin))
    r = {"Il": Il, "Ir": Ir, "costl": cost(Il, Ir, PDMINL), "costr": cost(Ir, Il, 0)}
    r["aggl"], r["aggr"] = ref.aggregate(rgb_l, r["costl"]), ref.aggregate(rgb_r, r["costr"])
    sl, sr = ref.states(r["aggl"]), ref.states(r["aggr"])
    r["keys"] = np.stack((sl["keys"], sr["keys"]))
    r["bestl"], r["bestr"] = sl["best"], sr["best"]
    r["dmapl"], r["dmapr"] = subpix_ref.dmap_of(sl["z"], sl["best"], PDMINL), subpix_ref.dmap_of(sr["z"], sr["best"], 0)
    r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], PDMINL - 100)
    r["unique"], r["margin"] = uniq_ref.apply(r["occlusion"], sl["z"] >= 0, sl["best"], sl["uq"][0], RATIO, PDMINL, PDMINL - 100)
    r["despeckled"] = speckle_ref.speckle_filter(r["unique"], float(PDMINL), float(PDMINL - 100), *SPK)
    r["filled"] = orc.fill_occlusion(r["despeckled"], PDMINL)
    mode = subpix_ref.MODES["parabola"]
    r["subpixl"], r["subpix_filled"] = subpix_ref.maps(mode, sl["z"], sl["best"], sl["nbr"][0], sl["nbr"][1], r["dmapl"],
                                                       r["despeckled"], r["filled"], PDMINL)
    r["subpixr"], _ = subpix_ref.maps(mode, sr["z"], sr["best"], sr["nbr"][0], sr["nbr"][1], r["dmapr"])
    wp = smx.default_wmf_params()
    ws, wc = smx.wmf_weights(wp)
    r["refined"] = wmf_ref.weighted_median(Il, r["filled"], PDMINL, PD, r["despeckled"], wp.radius, ws, wc)
    return r


@pytest.fixture(scope="module")
def colour_scene(orc):
    rgb_l, rgb_r = ref.colour_pair(PW, PH, PD, 4711)
    return rgb_l, rgb_r, {census: chain(orc, rgb_l, rgb_r, census) for census in (False, True)}


@pytest.fixture(scope="module")
def adcensus_want(colour_scene, orc):
    return chain(orc, colour_scene[0], colour_scene[1], "adcensus")


def _pipe(rgb_l, rgb_r, Il, Ir, **kw):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, **kw)
    t = lambda a: torch.from_numpy(a).cuda()
    if kw.get("guidance"):
        pipe.run(t(Il), t(Ir), rgb_l=t(rgb_l), rgb_r=t(rgb_r))
    else:
        pipe.run(t(Il), t(Ir))
    return pipe


ALL_STAGES = dict(subpixel="parabola", uniqueness=RATIO, wmf="occluded", want_agg=True)
CHAIN_KEYS = ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "unique", "margin", "despeckled", "filled",
              "subpixl", "subpixr", "subpix_filled", "refined")


@pytest.mark.parametrize("census", [False, True])
@pytest.mark.parametrize("sif", [None, 5])
def test_pipeline(colour_scene, census, sif):
    rgb_l, rgb_r, wants = colour_scene
    want = wants[census]
    pipe = _pipe(rgb_l, rgb_r, want["Il"], want["Ir"], guidance="rgb", cost="census" if census else None, speckle=_spk(),
                 slices_in_flight=sif, **ALL_STAGES)
    assert pipe.cgf_ws is not None and pipe.ws_bytes == 0 and pipe.slices_in_flight == (PD if sif is None else sif)
    got = pipe.results()
    for k in CHAIN_KEYS:
        _eq(got[k], want[k], k)
    _eq(pipe.keys.cpu().numpy(), want["keys"], "keys")
    assert not got["meanl"].any() and not got["meanr"].any()
    assert np.any(want["despeckled"] != want["unique"]) and np.any(want["unique"] != want["occlusion"])
    assert np.any(want["refined"] != want["filled"])


def test_pipeline_takes_cost_volumes_and_a_graph_replay_gives_the_same_bits(colour_scene, orc):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    rgb_l, rgb_r, wants = colour_scene
    want = wants[False]
    t = lambda a: torch.from_numpy(a).cuda()
    Il, Ir, rl, rr = t(want["Il"]), t(want["Ir"]), t(rgb_l), t(rgb_r)
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, guidance="rgb", want_agg=True, slices_in_flight=6)
    cl, cr = t(orc.cost_volume(want["Il"], want["Ir"], PD, PDMINL)), t(orc.cost_volume(want["Ir"], want["Il"], PD, 0))
    pipe.aggregate(Il, Ir, cl, cr, rgb_l=rl, rgb_r=rr)
    pipe.finish()
    got = pipe.results()
    for k in ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion"):
        _eq(got[k], want[k], "given volumes " + k)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pipe.run(Il, Ir, rgb_l=rl, rgb_r=rr)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pipe.run(Il, Ir, rgb_l=rl, rgb_r=rr)
        for x in (pipe.keys, pipe.agg, pipe.filled, pipe.dmap):
            x.zero_()
        g.replay()
    torch.cuda.current_stream().wait_stream(s)
    r2 = pipe.results()
    for k in got:
        _eq(r2[k], got[k], "replay " + k)


def test_pipeline_refusals(colour_scene):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    rgb_l, rgb_r, wants = colour_scene
    t = lambda a: torch.from_numpy(a).cuda()
    Il, Ir = t(wants[False]["Il"]), t(wants[False]["Ir"])
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, guidance="colour")
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, guidance="rgb", aggregation="sgm")
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, guidance="rgb")
    with pytest.raises(ValueError):
        pipe.run(Il, Ir)                                          # a missing guide
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=t(rgb_l))
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=t(rgb_l), rgb_r=t(rgb_r[:, :, 0]))
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, dminl=PDMINL).aggregate(Il, Ir, rgb_l=t(rgb_l), rgb_r=t(rgb_r))


def test_guidance_none_changes_nothing(colour_scene):
    rgb_l, rgb_r, wants = colour_scene
    Il, Ir = wants[False]["Il"], wants[False]["Ir"]
    for kw in ({}, dict(cost="census", subpixel="parabola", uniqueness=RATIO, want_agg=True)):
        a = _pipe(rgb_l, rgb_r, Il, Ir, guidance=None, **kw)
        assert a.guidance is None and a.cgf_ws is None and a.cgf_cost is None and a.cgf_ws_bytes == 0
        b = _pipe(rgb_l, rgb_r, Il, Ir, **kw)
        ra, rb = a.results(), b.results()
        assert ra.keys() == rb.keys() and a.ws_bytes == b.ws_bytes and a.slices_in_flight == b.slices_in_flight
        for k in ra:
            _eq(ra[k], rb[k], k)


def test_the_isoluminant_step_survives_the_pipeline(orc):
    """After finish, the disparity step of the isoluminant scene sits at x = 32 with guidance="rgb"."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    rgb, p, _ = ref.isoluminant_scene(orc.gray)
    h, w = rgb.shape[:2]
    cost = np.concatenate((p, 1 - p)).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    g = t(orc.gray(rgb))
    pipe = PairPipeline(w, h, 2, dminl=0, guidance="rgb")
    pipe.aggregate(g, g, t(cost), t(cost), rgb_l=t(rgb), rgb_r=t(rgb))
    pipe.finish()
    dmap = pipe.results()["dmapl"]
    assert (dmap[:, :32] == 0).all() and (dmap[:, 32:] == 1).all()
    step = np.flatnonzero(np.diff(dmap[h // 2]))
    assert step.tolist() == [31]                                  # between x = 31 and x = 32, nowhere else


def _ctx_pair(ctx, entry, imgs, channels, want_vol, mean=False):
    L, n = smx.lib(), PW * PH
    bufs = {k: np.empty((PH, PW), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if want_vol:
        for k in ("agg_l", "agg_r", "cost_l", "cost_r"):
            bufs[k] = np.empty((PD, PH, PW), np.float32)
    if mean:
        bufs["mean_l"] = np.empty((PH, PW), np.uint8)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    args = (imgs[0].ctypes.data, imgs[1].ctypes.data) + ((channels,) if channels else ()) + (PDMINL, 0, C.byref(out))
    return entry(ctx, *args), bufs


CTX_NAMES = (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"), ("occlusion", "occlusion"),
             ("filled", "filled"))
CTX_VOLUMES = (("agg_l", "aggl"), ("agg_r", "aggr"), ("cost_l", "costl"), ("cost_r", "costr"))


def _ctx_create():
    ctx = C.c_void_p()
    _lib.check(smx.lib().smx_create(C.byref(smx.default_params()), PW, PH, PD, C.byref(ctx)))
    return ctx


def _check_ctx_stages(ctx, got, want, want_vol, label):
    """The planes and the maps of a context pair that ran with sub-pixel, uniqueness and speckle removal on, against `chain`"""
    L = smx.lib()
    for k, name in CTX_NAMES + ((("agg_l", "aggl"), ("agg_r", "aggr")) if want_vol else ()):
        _eq(got[k], want[name], f"{label} {name} (volumes {want_vol})")
    sub = [np.empty((PH, PW), np.float32) for _ in range(3)]
    _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
    for s, name in zip(sub, ("subpixl", "subpixr", "subpix_filled")):
        _eq(s, want[name], f"{label} {name}")
    desp, uni, margin = (np.empty((PH, PW), np.float32) for _ in range(3))
    _lib.check(L.smx_ctx_speckle_map(ctx, desp.ctypes.data))
    _lib.check(L.smx_ctx_uniqueness_map(ctx, uni.ctypes.data, margin.ctypes.data))
    _eq(desp, want["despeckled"], label + " despeckled")
    _eq(uni, want["unique"], label + " unique")
    _eq(margin, want["margin"], label + " margin")


@pytest.mark.parametrize("census", [False, True])
def test_context(colour_scene, orc, census):
    rgb_l, rgb_r, wants = colour_scene
    want = wants[census]
    L = smx.lib()
    ctx = _ctx_create()
    try:
        assert L.smx_ctx_set_guidance(ctx, 2) == -1
        if census:
            _lib.check(L.smx_ctx_set_cost(ctx, 1, None))
        # GRAY mode: the rgb entry equals smx_ctx_stereo_pair on the converted images
        rc, a = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 3, True, mean=True)
        _lib.check(rc)
        rc, b = _ctx_pair(ctx, L.smx_ctx_stereo_pair, (want["Il"], want["Ir"]), 0, True, mean=True)
        _lib.check(rc)
        for k in a:
            _eq(a[k], b[k], "gray mode " + k)
        # RGB mode with every later stage: the pipeline's (= the references') outputs
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        assert L.smx_ctx_stereo_pair_async(ctx, want["Il"].ctypes.data, want["Ir"].ctypes.data, PDMINL, 0) == -1
        assert b"guidance" in L.smx_last_error()           # (before the later stages, which the async entry refuses as well)
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, RATIO))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk())))
        for want_vol in (True, False):
            rc, got = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 3, want_vol)
            _lib.check(rc)
            _check_ctx_stages(ctx, got, want, want_vol, "ctx")
        # four channels: the same bits
        rgba = [np.concatenate((x, np.full((PH, PW, 1), 9, np.uint8)), axis=2) for x in (rgb_l, rgb_r)]
        rc, got4 = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, rgba, 4, False)
        _lib.check(rc)
        for k in got4:
            _eq(got4[k], got[k], "rgba " + k)
        # the refusals
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 3, False, mean=True)
        assert rc == -1 and b"mean" in L.smx_last_error()
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair, (want["Il"], want["Ir"]), 0, False)
        assert rc == -1 and b"smx_ctx_stereo_pair_rgb" in L.smx_last_error()
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 5, False)
        assert rc == -1
        _lib.check(L.smx_ctx_set_aggregation(ctx, 1, None))
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 3, False)
        assert rc == -1 and b"semi-global" in L.smx_last_error()
    finally:
        L.smx_destroy(ctx)


@pytest.mark.parametrize("cost", [None, "adcensus"])
def test_context_chunks_do_not_change_a_bit(colour_scene, adcensus_want, orc, cost):
    """The context's chunk loop under smx_set_max_slices_per_launch: 5 gives chunks of 5, 5, 5 and a ragged last one of a single
    slice, 16 one chunk, 1 every slice alone.  With the volumes the chunks go view by view into the whole volumes at their
    slice offsets; without them in the pair form from the chunk buffer.  Everything against the numpy references of the
    fixtures; without the later stages the filled map is the fill of the occlusion map."""
    rgb_l, rgb_r, wants = colour_scene
    want = dict(adcensus_want if cost == "adcensus" else wants[False])
    want["filled"] = orc.fill_occlusion(want["occlusion"], PDMINL)
    L = smx.lib()
    ctx = _ctx_create()
    try:
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        if cost == "adcensus":
            _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
        for k in (1, 5, 16):
            for want_vol in (True, False):
                _lib.check(L.smx_set_max_slices_per_launch(k))
                try:
                    rc, got = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, (rgb_l, rgb_r), 3, want_vol)
                finally:
                    L.smx_set_max_slices_per_launch(0)
                _lib.check(rc)
                for key, name in CTX_NAMES + (CTX_VOLUMES if want_vol else ()):
                    _eq(got[key], want[name], f"ctx cost {cost}, at most {k} slices, volumes {want_vol}: {name}")
    finally:
        L.smx_destroy(ctx)
