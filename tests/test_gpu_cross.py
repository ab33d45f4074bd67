"""Cross-based aggregation on the GPU (smx_dev_cross_arms, smx_dev_cross_wta_pair, smx_cross_aggregate,
PairPipeline(aggregation="cross"), smx_ctx_set_cross), bit for bit against the numpy reference of tests/cross_ref.py.  Every
device call hands its buffers over inside guard bands (tests/guarded.py) with the workspace poisoned and off its alignment, so
each case checks the memory contract too.

k_cross_h emits strips of 128 columns from 256 staged ones, k_cross_v takes 64 columns a workgroup and keeps 2 * l1 + 2 rows in
its ring, k_cross_arms takes 256 columns of a row: the shapes aim at those edges.

Run on the GPU box:  python -m pytest tests -m gpu -q -k cross
"""
import ctypes as C
import functools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import adcensus_ref
import census_ref
import cgf_ref
import cross_ref as ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

MEI = dict(l1=34, l2=17, tau1=20, tau2=6, iterations=4)


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


def _p(**kw):
    p = smx.default_cross_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _kw(p, arms_only=False):
    """the parameters as the keywords of cross_ref"""
    kw = dict(l1=p.l1, l2=p.l2, tau1=p.tau1, tau2=p.tau2)
    if not arms_only:
        kw["iterations"] = p.iterations
    return kw


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _guide(kind, w, h, view, channels=3):
    """(h, w, channels) uint8, read-only; a fourth byte is random"""
    rng = np.random.default_rng(500 * w + h + view)
    if kind == "constant":
        g = np.empty((h, w, channels), np.uint8)
        g[:] = rng.integers(0, 256, channels, dtype=np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], channels, axis=2)
    elif kind == "textured":
        # blocks in nearby colours with noise: arms of every length, cut by either threshold
        blocks = rng.integers(90, 120, ((h + 7) // 8, (w + 7) // 8, channels))
        g = (np.kron(blocks, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w, channels))).astype(np.uint8)
    else:
        g = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
    if channels == 4:
        g = g.copy()
        g[:, :, 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _costs(kind, w, h, D, view):
    """(D, h, w) float32, read-only"""
    rng = np.random.default_rng(1000 * w + 10 * h + D + view)
    if kind == "floats":
        c = (rng.random((D, h, w)) * 255).astype(np.float32)
    elif kind == "full":
        c = rng.choice(np.array([255.0, 255.5, 300.0, 1e9, np.inf], np.float32), (D, h, w))      # every one clamps to 255
    elif kind == "special":
        c = (rng.random((D, h, w)) * 300 - 30).astype(np.float32)
        flat = c.reshape(-1)
        idx = rng.permutation(flat.size)
        specials = np.array([np.nan, np.inf, -np.inf, -0.0, -1e30, 1e30, 255.0, 255.5, 256.0, 0.999], np.float32)
        for k, s in enumerate(specials):
            flat[idx[k::len(specials)][:max(1, flat.size // 40)]] = s
        flat[idx[0]] = np.nan           # (a 1 x 1 x 1 volume holds a NaN)
    else:
        ww = max(w, 16)                 # (the census window and the shift want some columns)
        Il, Ir = synth.gen_pair(ww, h, D, 77 + w + h)
        a, b, dmin = (Il, Ir, 1 - D) if view == 0 else (Ir, Il, 0)
        c = census_ref.census_cost(a, b, D, dmin) if kind == "census" else adcensus_ref.gray_cost(a, b, D, dmin)
        c = np.ascontiguousarray(c[:, :, :w], np.float32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=64)
def _want_cached(gkind, ckind, w, h, D, view, channels, params):
    q = ref.aggregate(_guide(gkind, w, h, view, channels), _costs(ckind, w, h, D, view), **dict(params))
    q.setflags(write=False)
    return q


def _want(gkind, ckind, w, h, D, view, p, channels=3):
    return _want_cached(gkind, ckind, w, h, D, view, channels, tuple(sorted(_kw(p).items())))


# ---------------------------------------------------------------------------------------------
# arms
# ---------------------------------------------------------------------------------------------
def _arms(p, gl, gr, misalign=0):
    """smx_dev_cross_arms on guarded buffers -> (views, h, w) uint32"""
    some = gl if gl is not None else gr
    h, w, ch = some.shape
    V = (gl is not None) + (gr is not None)
    gg = [None if g is None else Guarded(g.nbytes, np.uint8, g.shape, plane=w * h, misalign=3).load(g) for g in (gl, gr)]
    out = Guarded(V * w * h * 4, np.uint8, (V * w * h * 4,), plane=w * h, misalign=misalign)
    ptr = lambda g: None if g is None else g.ptr
    _lib.check(smx.lib().smx_dev_cross_arms(C.byref(p), ptr(gg[0]), ptr(gg[1]), ch, w, h, out.ptr, _stream()))
    out.check("d_arms")
    for g in gg:
        if g is not None:
            g.check_unchanged("a guide")
    return out.numpy().view(np.uint32).reshape(V, h, w)


ARM_PARAMS = [dict(l1=l1, l2=l2, tau1=t1, tau2=t2) for l1 in (1, 17, 63) for l2 in sorted({0, l1})
              for t1, t2 in ((1, 1), (20, 6), (256, 256), (256, 1))]


@pytest.mark.parametrize("h", [1, 2, 70])
@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 129])
def test_arms(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    border = np.stack((xx, w - 1 - xx, yy, h - 1 - yy))
    for ch in (1, 3, 4):
        for kind in ("constant", "checker", "textured"):
            gl, gr = _guide(kind, w, h, 0, ch), _guide(kind, w, h, 1, ch)
            for kw in ARM_PARAMS:
                got = _arms(_p(**kw), gl, gr)
                for v, g in enumerate((gl, gr)):
                    if kind == "constant" or kw["tau2"] == 256:
                        want = np.minimum(kw["l1"], border).astype(np.int32)          # the arms clip at the borders only
                    elif kind == "checker" and kw["tau1"] < 256:
                        want = np.zeros((4, h, w), np.int32)                            # every arm is 0
                    else:
                        want = ref.arms(g, **kw)
                    _eq(got[v], ref.pack_arms(want), f"{w}x{h} ch{ch} {kind} {kw} view {v}")


def test_arms_one_view_forms_and_alignment():
    w, h = 129, 70
    gl, gr = _guide("textured", w, h, 0), _guide("textured", w, h, 1)
    p = _p()
    both = _arms(p, gl, gr)
    _eq(_arms(p, gl, None, misalign=4)[0], both[0], "left alone")
    _eq(_arms(p, None, gr, misalign=252)[0], both[1], "right alone")
    assert len(np.unique(both & 255)) > 10


# ---------------------------------------------------------------------------------------------
# aggregation
# ---------------------------------------------------------------------------------------------
class Call:
    """The buffers of smx_dev_cross_wta_pair calls on one pair, every one guarded.  guide_*: (h, w, ch) uint8 or None,
    cost_*: (D, h, w) float32 or None; a call covers slices [s0, s1) of them."""

    def __init__(self, guide_l, cost_l, guide_r, cost_r, ws_slices=None, misalign=13, slots=None):
        self.guides, self.costs = (guide_l, guide_r), (cost_l, cost_r)
        some = cost_l if cost_l is not None else cost_r
        D, h, w = some.shape
        self.D, self.h, self.w, self.n = D, h, w, w * h
        self.ch = (guide_l if guide_l is not None else guide_r).shape[2]
        self.nviews = (cost_l is not None) + (cost_r is not None)
        slots = self.nviews if slots is None else slots
        n = self.n
        self.gguide = [None if g is None else Guarded(g.nbytes, np.uint8, g.shape, plane=n, misalign=3).load(g) for g in self.guides]
        self.gcost = [None if c is None else Guarded(c.nbytes, np.float32, c.shape, plane=n).load(c) for c in self.costs]
        self.keys = Guarded(slots * n * 8, np.int64, (slots, h, w), plane=n)
        self.agg = Guarded(slots * D * n * 4, np.float32, (slots, D, h, w), plane=n)
        self.nbr = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.uq = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.ws_bytes = smx.lib().smx_cross_workspace_bytes(w, h, D if ws_slices is None else ws_slices, self.nviews)
        assert self.ws_bytes > 0
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)
        self.poison()
        self.init_keys()

    def poison(self, byte=0xC3):
        self.ws.view.fill_(byte)                    # the call may rely on nothing in here

    def init_keys(self):
        self.keys.view.fill_(np.iinfo(np.int64).max)

    def run(self, p, s0=0, s1=None, ws_bytes=None, agg=True, nbr=True, uq=True):
        s1 = self.D if s1 is None else s1
        ptr = lambda g: None if g is None else g.ptr
        off = lambda g, b: None if g is None else C.c_void_p(g.ptr.value + b)
        # d_cost / d_agg of a call start at its first slice
        return smx.lib().smx_dev_cross_wta_pair(
            C.byref(p), ptr(self.gguide[0]), ptr(self.gguide[1]), self.ch, off(self.gcost[0], s0 * self.n * 4),
            off(self.gcost[1], s0 * self.n * 4), self.w, self.h, s0, s1, self.keys.ptr, self.agg.ptr if agg else None,
            self.nbr.ptr if nbr else None, self.uq.ptr if uq else None, self.ws.ptr,
            self.ws_bytes if ws_bytes is None else ws_bytes, _stream())

    def check_memory(self):
        for g, name in ((self.keys, "d_keys"), (self.agg, "d_agg"), (self.nbr, "d_nbr"), (self.uq, "d_uq"), (self.ws, "d_ws")):
            g.check(name)
        for g in self.gguide + self.gcost:
            if g is not None:
                g.check_unchanged("an input")

    def check_outputs(self, wants, label="", agg=True, nbr=True, uq=True):
        """wants: the aggregated volume of every view of the call, in order; the states against subpix_ref / uniq_ref on it"""
        self.check_memory()
        keys, got, gn, gu = self.keys.numpy(), self.agg.numpy(), self.nbr.numpy(), self.uq.numpy()
        for slot, q in enumerate(wants):
            st = cgf_ref.states(q)
            if agg:
                _eq(got[slot], q, f"{label} agg[{slot}]")
            _eq(keys[slot], st["keys"], f"{label} keys[{slot}]")
            if nbr:
                _eq(gn[slot], st["nbr"], f"{label} nbr[{slot}]")
            if uq:
                _eq(gu[slot], st["uq"], f"{label} uq[{slot}]")


def _pair(gkind, ckind, w, h, D, channels=3, **kw):
    return Call(_guide(gkind, w, h, 0, channels), _costs(ckind, w, h, D, 0), _guide(gkind, w, h, 1, channels),
                _costs(ckind, w, h, D, 1), **kw)


# 20 rows: below l1 = 34; 150 rows: above 2 * 34 + 2, so the ring of the default arm length wraps (70 rows do for l1 = 17)
SHAPES = [(1, 1, 1), (5, 3, 2), (129, 70, 5), (300, 40, 3), (70, 20, 2), (33, 150, 2)]
PARAMS = [MEI, dict(l1=17, l2=8, tau1=20, tau2=6, iterations=3), dict(l1=5, l2=0, tau1=256, tau2=256, iterations=2),
          dict(l1=63, l2=63, tau1=30, tau2=30, iterations=1)]


@pytest.mark.parametrize("ckind", ["floats", "census", "adcensus", "special"])
@pytest.mark.parametrize("w,h,D", SHAPES)
def test_against_the_reference(w, h, D, ckind):
    for gkind, ch in (("textured", 3), ("random", 1), ("constant", 4)):
        call = _pair(gkind, ckind, w, h, D, channels=ch)
        for kw in PARAMS:
            p = _p(**kw)
            call.poison()
            call.init_keys()
            _lib.check(call.run(p))
            with np.errstate(all="ignore"):
                call.check_outputs([_want(gkind, ckind, w, h, D, v, p, ch) for v in (0, 1)], f"{w}x{h}x{D} {ckind} {gkind} {kw}")


@pytest.mark.parametrize("iterations", [1, 2, 3, 4])
def test_the_largest_sums(iterations):
    """l1 = 63 on a constant guide, costs at and above the clamp: regions of 127 x 127 pixels of 4080"""
    w, h, D = 140, 131, 1
    p = _p(l1=63, l2=63, tau1=20, tau2=6, iterations=iterations)
    call = _pair("constant", "full", w, h, D)
    _lib.check(call.run(p))
    wants = [_want("constant", "full", w, h, D, v, p) for v in (0, 1)]
    call.check_outputs(wants, f"{iterations} iterations")
    a = ref.arms(_guide("constant", w, h, 0), **_kw(p, arms_only=True))
    assert ref.areas(a).max() == 127 * 127 and wants[0].min() == 255.0 == wants[0].max()      # S = 127^2 * 4080


@pytest.mark.parametrize("left", [True, False])
def test_one_view_forms_leave_the_other_view_alone(left):
    for (w, h, D), kw in (((129, 70, 5), MEI), ((33, 150, 2), PARAMS[1]), ((5, 3, 2), PARAMS[2])):
        v = 0 if left else 1
        p = _p(**kw)
        g, c = _guide("textured", w, h, v), _costs("floats", w, h, D, v)
        call = Call(g if left else None, c if left else None, None if left else g, None if left else c, slots=2)
        _lib.check(call.run(p))
        call.check_outputs([_want("textured", "floats", w, h, D, v, p)], "one view")
        assert bool((call.keys.view[1] == np.iinfo(np.int64).max).all()), "keys: the second view's half was written"
        for buf, name in ((call.agg, "agg"), (call.nbr, "nbr"), (call.uq, "uq")):
            assert bool((buf.bytes[buf.nbytes // 2:] == buf.fill).all()), f"{name}: the second view's half was written by a one-view call"


@pytest.mark.parametrize("agg,nbr,uq", [(False, False, False), (True, False, False), (False, True, False), (False, False, True),
                                        (True, True, False), (False, True, True), (True, True, True)])
def test_optional_outputs_alone_and_together(agg, nbr, uq):
    w, h, D = 129, 70, 5
    p = _p()
    wants = [_want("textured", "adcensus", w, h, D, v, p) for v in (0, 1)]
    for misalign in (0, 1, 255):
        call = _pair("textured", "adcensus", w, h, D, misalign=misalign)
        _lib.check(call.run(p, agg=agg, nbr=nbr, uq=uq))
        call.check_outputs(wants, f"agg {agg} nbr {nbr} uq {uq}, misalign {misalign}", agg=agg, nbr=nbr, uq=uq)
        for on, g, name in ((agg, call.agg, "d_agg"), (nbr, call.nbr, "d_nbr"), (uq, call.uq, "d_uq")):
            if not on:
                g.check_untouched(name + " (not requested)")


def test_the_tie_rule_on_a_volume_of_equal_slices():
    w, h, D = 65, 9, 4
    g = _guide("textured", w, h, 0)
    cost = np.repeat(_costs("floats", w, h, 1, 0), D, axis=0)
    call = Call(g, cost, g, cost)
    p = _p()
    _lib.check(call.run(p))
    call.check_outputs([ref.aggregate(g, cost, **_kw(p))] * 2, "equal slices")
    assert bool(((call.keys.view & 0xFFFFFFFF) == 0xFFFFFFFF - (D - 1)).all())     # the last slice wins everywhere


# ---------------------------------------------------------------------------------------------
# chunking
# ---------------------------------------------------------------------------------------------
W, H, D = 129, 70, 5


@pytest.fixture(scope="module")
def wants():
    return [_want("textured", "adcensus", W, H, D, v, _p()) for v in (0, 1)]


@pytest.mark.parametrize("ws_slices", [1, 2, D])
def test_the_workspace_size_does_not_change_a_bit(wants, ws_slices):
    call = _pair("textured", "adcensus", W, H, D, ws_slices=ws_slices)
    _lib.check(call.run(_p()))
    call.check_outputs(wants, f"workspace for {ws_slices} slices")


def test_max_slices_per_launch_does_not_change_a_bit(wants):
    call = _pair("textured", "adcensus", W, H, D)
    L = smx.lib()
    try:
        for k in (1, 2):
            _lib.check(L.smx_set_max_slices_per_launch(k))
            call.poison()
            call.init_keys()
            _lib.check(call.run(_p()))
            call.check_outputs(wants, f"max slices per launch {k}")
    finally:
        L.smx_set_max_slices_per_launch(0)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_two_slice_ranges_on_one_set_of_keys_against_one_call(wants, k):
    call = _pair("textured", "adcensus", W, H, D, ws_slices=2)
    _lib.check(call.run(_p(), 0, k))
    call.poison(0x3C)
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
    """IN/OUT keys: a call on keys that hold a better winner of another shard keeps it."""
    call = _pair("textured", "adcensus", W, H, D)
    best = smx.lib().smx_pack_key(-1.0, 2)
    call.keys.view.fill_(best)
    _lib.check(call.run(_p(), nbr=False, uq=False))
    assert bool((call.keys.view == best).all())
    call.check_memory()


# ---------------------------------------------------------------------------------------------
# runtime and memory behaviour
# ---------------------------------------------------------------------------------------------
def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    w, h, d = 19, 40, 3
    call = _pair("textured", "floats", w, h, d, ws_slices=1)
    call.ws.view.fill_(call.ws.fill)
    call.keys.bytes.fill_(call.keys.fill)
    assert call.run(_p(), ws_bytes=call.ws_bytes - 1) == -3
    assert b"workspace" in smx.lib().smx_last_error()
    for g, name in ((call.keys, "d_keys"), (call.agg, "d_agg"), (call.nbr, "d_nbr"), (call.uq, "d_uq"), (call.ws, "d_ws")):
        g.check_untouched(name)
    call.init_keys()
    call.poison()
    _lib.check(call.run(_p()))                       # ... and exactly that many bytes are enough
    call.check_outputs([_want("textured", "floats", w, h, d, v, _p()) for v in (0, 1)], "smallest workspace")


def test_two_runs_and_a_graph_replay_give_the_same_bits(wants):
    import torch
    call = _pair("textured", "adcensus", W, H, D, ws_slices=2)
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


def test_host_pointer_entry():
    w, h, d = 45, 11, 6
    p = _p(l1=9, l2=4, iterations=2)
    for ch in (1, 3):
        g, cost = _guide("textured", w, h, 0, ch), _costs("floats", w, h, d, 0)
        best, dmap = smx.init_wta(h, w)
        agg = smx.cross_aggregate(g[:, :, 0] if ch == 1 else g, cost, best, dmap, -5, want_agg=True, params=p)
        q = ref.aggregate(g, cost, **_kw(p))
        st = cgf_ref.states(q)
        _eq(agg, q, "agg")
        _eq(best, st["best"], "filter_cost")
        _eq(dmap, (st["z"] - 5).astype(np.float32), "disp_map")
    # IN/OUT like the reference's: a pixel is updated iff filter_cost >= min q
    best2 = np.full((h, w), -1.0, np.float32)
    dmap2 = np.full((h, w), 3.0, np.float32)
    assert smx.cross_aggregate(g, cost, best2, dmap2, -5, params=p) is None
    assert (best2 == -1).all() and (dmap2 == 3).all()
    # the defaults
    best, dmap = smx.init_wta(h, w)
    _eq(smx.cross_aggregate(g, cost, best, dmap, 0, want_agg=True), ref.aggregate(g, cost), "defaults")


# ---------------------------------------------------------------------------------------------
# the reason for the feature
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_the_step_between_two_colours_of_equal_luminance_on_the_gpu(iterations):
    g, cost, truth = ref.step_scene(seed=1)
    h, w = truth.shape
    best, dmap = smx.init_wta(h, w)
    smx.cross_aggregate(g, cost, best, dmap, 0, params=_p(l1=17, l2=8, tau1=20, tau2=6, iterations=iterations))
    assert np.array_equal(dmap, truth.astype(np.float32))
    best, dmap = smx.init_wta(h, w)
    smx.cross_aggregate(g, cost, best, dmap, 0, params=_p(l1=17, l2=8, tau1=256, tau2=256, iterations=iterations))
    assert np.any(dmap != truth)


# ---------------------------------------------------------------------------------------------
# the pipeline and the context
# ---------------------------------------------------------------------------------------------
PW, PH, PD, PDMINL = 129, 70, 16, -15
SPK = (30, 1.0)
RATIO = 0.15
PIPE_PARAMS = dict(l1=17, l2=8, tau1=20, tau2=6, iterations=2)
ALL_STAGES = dict(subpixel="parabola", uniqueness=RATIO, wmf="occluded", want_agg=True)
MAPS = ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")
CHAIN_KEYS = ("aggl", "aggr") + MAPS + ("unique", "margin", "despeckled", "subpixl", "subpixr", "subpix_filled", "refined")


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def chain(orc, Il, aggl, aggr):
    """The later stages from the aggregated volumes of both views, in numpy"""
    import speckle_ref
    import subpix_ref
    import uniq_ref
    import wmf_ref
    r = {"aggl": aggl, "aggr": aggr}
    sl, sr = cgf_ref.states(aggl), cgf_ref.states(aggr)
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
def scene(orc):
    """A colour pair, its gray images, the three costs of both views, and per (cost, guide) the aggregated volumes"""
    rgb_l, rgb_r = cgf_ref.colour_pair(PW, PH, PD, 4711)
    Il, Ir = orc.gray(rgb_l), orc.gray(rgb_r)
    cost = {None: (orc.cost_volume(Il, Ir, PD, PDMINL), orc.cost_volume(Ir, Il, PD, 0)),
            "census": (census_ref.census_cost(Il, Ir, PD, PDMINL), census_ref.census_cost(Ir, Il, PD, 0)),
            "adcensus": (adcensus_ref.gray_cost(Il, Ir, PD, PDMINL), adcensus_ref.gray_cost(Ir, Il, PD, 0))}
    guides = {"gray": (Il[:, :, None], Ir[:, :, None]), "rgb": (rgb_l, rgb_r)}
    agg = {(c, g): tuple(ref.aggregate(guides[g][v], cost[c][v], **PIPE_PARAMS) for v in (0, 1)) for c in cost for g in guides}
    return dict(rgb=(rgb_l, rgb_r), Il=Il, Ir=Ir, cost=cost, agg=agg)


def _pipe(scene, guide, run=True, **kw):
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="cross", cross_params=_p(**PIPE_PARAMS), **kw)
    if run:
        if guide == "rgb":
            pipe.run(_t(scene["Il"]), _t(scene["Ir"]), rgb_l=_t(scene["rgb"][0]), rgb_r=_t(scene["rgb"][1]))
        else:
            pipe.run(_t(scene["Il"]), _t(scene["Ir"]))
    return pipe


@pytest.mark.parametrize("guide", ["gray", "rgb"])
@pytest.mark.parametrize("cost", [None, "census", "adcensus"])
def test_pipeline(orc, scene, cost, guide):
    import subpix_ref
    aggl, aggr = scene["agg"][(cost, guide)]
    sl, sr = cgf_ref.states(aggl), cgf_ref.states(aggr)
    want = {"aggl": aggl, "aggr": aggr, "bestl": sl["best"], "bestr": sr["best"],
            "dmapl": subpix_ref.dmap_of(sl["z"], sl["best"], PDMINL), "dmapr": subpix_ref.dmap_of(sr["z"], sr["best"], 0)}
    want["occlusion"] = orc.detect_occlusion(want["dmapl"], want["dmapr"], PDMINL - 100)
    want["filled"] = orc.fill_occlusion(want["occlusion"], PDMINL)
    for sif in (None, 5):
        pipe = _pipe(scene, guide, cost=cost, want_agg=True, slices_in_flight=sif)
        assert pipe.cross_ws is not None and pipe.ws_bytes == 0 and pipe.slices_in_flight == (PD if sif is None else sif)
        assert (pipe.cross_cost is None) == (cost is not None)
        got = pipe.results()
        for k in want:
            _eq(got[k], want[k], f"cost {cost} guide {guide} sif {sif} {k}")
        _eq(pipe.keys.cpu().numpy(), np.stack((sl["keys"], sr["keys"])), "keys")
        assert not got["meanl"].any() and not got["meanr"].any()
    assert len(np.unique(want["dmapl"])) > 3


def test_composition_with_subpixel_uniqueness_speckle_and_weighted_median(orc, scene):
    want = chain(orc, scene["Il"], *scene["agg"][("adcensus", "rgb")])
    pipe = _pipe(scene, "rgb", cost="adcensus", speckle=_spk(), slices_in_flight=6, **ALL_STAGES)
    got = pipe.results()
    for k in CHAIN_KEYS:
        _eq(got[k], want[k], k)
    _eq(pipe.keys.cpu().numpy(), want["keys"], "keys")
    assert np.any(want["unique"] != want["occlusion"]) and np.any(want["refined"] != want["filled"])
    assert np.any(want["subpixl"] != want["dmapl"])


def test_pipeline_slice_sub_ranges_and_given_volumes(orc, scene):
    """Two D-shards merged by the int64 min equal the whole range; the caller's volumes take the place of the cost build."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    aggl, aggr = scene["agg"][(None, "gray")]
    keys = np.stack((cgf_ref.states(aggl)["keys"], cgf_ref.states(aggr)["keys"]))
    Il, Ir = _t(scene["Il"]), _t(scene["Ir"])
    parts = []
    for s0, s1 in ((0, 7), (7, PD)):
        pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="cross", cross_params=_p(**PIPE_PARAMS), s_begin=s0, s_end=s1,
                            want_agg=True, slices_in_flight=3)
        pipe.aggregate(Il, Ir)
        torch.cuda.synchronize()
        _eq(pipe.agg[0].cpu().numpy(), aggl[s0:s1], f"agg of [{s0}, {s1})")
        parts.append(pipe.keys.clone())
    _eq(torch.minimum(parts[0], parts[1]).cpu().numpy(), keys, "merged keys")
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="cross", cross_params=_p(**PIPE_PARAMS), want_agg=True)
    cl, cr = scene["cost"]["adcensus"]
    pipe.aggregate(Il, Ir, _t(cl), _t(cr))
    pipe.finish()
    got = pipe.results()
    _eq(got["aggl"], scene["agg"][("adcensus", "gray")][0], "given volumes aggl")
    _eq(got["aggr"], scene["agg"][("adcensus", "gray")][1], "given volumes aggr")


def test_pipeline_refusals(scene):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = _t(scene["Il"]), _t(scene["Ir"])
    rl, rr = _t(scene["rgb"][0]), _t(scene["rgb"][1])
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, aggregation="cross", guidance="rgb")
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, aggregation="bogus")
    with pytest.raises(_lib.SmxError):
        PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="cross", cross_params=_p(l1=64)).run(Il, Ir)
    pipe = _pipe(scene, "gray", run=False)
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=rl)                         # one guide alone
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=rl, rgb_r=rr[:, :, 0])
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, _t(scene["cost"][None][0]))       # one volume alone
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, aggregation="cross", uniqueness=0.1, s_begin=1)


def test_aggregation_none_is_unchanged_against_the_oracle(orc, scene):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = scene["Il"], scene["Ir"]
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation=None)
    assert pipe.cross_params is None and pipe.cross_ws is None and pipe.cross_cost is None and pipe.cross_ws_bytes == 0
    pipe.run(_t(Il), _t(Ir))
    got = pipe.results()
    want = orc.stereo_pair(Il, Ir, PD, dminl=PDMINL, dminr=0)
    for k in ("meanl", "meanr") + MAPS:
        _eq(got[k], want[k], k)


def _ctx_pair(ctx, entry, imgs, channels, want_vol, mean=False):
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


def _ctx_want(orc, scene, cost, guide):
    """What a context pair with cross-based aggregation hands out, in numpy: the six planes and the four volumes (kept in the
    scene: every test of the context compares against the same arrays)"""
    key = ("ctx want", cost, guide)
    if key not in scene:
        import subpix_ref
        aggl, aggr = scene["agg"][(cost, guide)]
        sl, sr = cgf_ref.states(aggl), cgf_ref.states(aggr)
        want = {"aggl": aggl, "aggr": aggr, "costl": scene["cost"][cost][0], "costr": scene["cost"][cost][1],
                "bestl": sl["best"], "bestr": sr["best"],
                "dmapl": subpix_ref.dmap_of(sl["z"], sl["best"], PDMINL), "dmapr": subpix_ref.dmap_of(sr["z"], sr["best"], 0)}
        want["occlusion"] = orc.detect_occlusion(want["dmapl"], want["dmapr"], PDMINL - 100)
        want["filled"] = orc.fill_occlusion(want["occlusion"], PDMINL)
        scene[key] = want
    return scene[key]


def _check_ctx_stages(ctx, got, want, label):
    """The planes and the maps of a context pair that ran with sub-pixel, uniqueness and speckle removal on, against `chain`"""
    L = smx.lib()
    for k, name in CTX_NAMES:
        _eq(got[k], want[name], f"{label} {name}")
    sub = [np.empty((PH, PW), np.float32) for _ in range(3)]
    _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
    for s, name in zip(sub, ("subpixl", "subpixr", "subpix_filled")):
        _eq(s, want[name], f"{label} {name}")
    uni, margin = (np.empty((PH, PW), np.float32) for _ in range(2))
    _lib.check(L.smx_ctx_uniqueness_map(ctx, uni.ctypes.data, margin.ctypes.data))
    _eq(uni, want["unique"], label + " unique")
    _eq(margin, want["margin"], label + " margin")


def _ctx_create():
    ctx = C.c_void_p()
    _lib.check(smx.lib().smx_create(C.byref(smx.default_params()), PW, PH, PD, C.byref(ctx)))
    return ctx


def _bounded_pair(k, *args):
    """_ctx_pair with at most k slices per launch on this thread, checked"""
    L = smx.lib()
    _lib.check(L.smx_set_max_slices_per_launch(k))
    try:
        rc, got = _ctx_pair(*args)
    finally:
        L.smx_set_max_slices_per_launch(0)
    _lib.check(rc)
    return got


def test_context(orc, scene):
    L = smx.lib()
    ctx = _ctx_create()
    names = CTX_NAMES
    gray, rgb = (scene["Il"], scene["Ir"]), scene["rgb"]
    try:
        # off: the context is the oracle's pair
        rc, off = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        plain = orc.stereo_pair(*gray, PD, dminl=PDMINL, dminr=0)
        for k, name in names:
            _eq(off[k], plain[name], "off " + name)
        for bad in (dict(l1=64), dict(l2=-1), dict(tau2=21), dict(iterations=0)):
            assert L.smx_ctx_set_cross(ctx, C.byref(_p(**bad))) == -1
        assert L.smx_ctx_set_aggregation(ctx, 2, None) == -1
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(_p(**PIPE_PARAMS))))
        assert L.smx_ctx_stereo_pair_async(ctx, gray[0].ctypes.data, gray[1].ctypes.data, PDMINL, 0) == -1
        assert b"smx_ctx_set_cross" in L.smx_last_error()
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False, mean=True)
        assert rc == -1 and b"mean" in L.smx_last_error()
        # on, with every cost, both guides, with and without the volumes
        for cost in (None, "census", "adcensus"):
            if cost == "census":
                _lib.check(L.smx_ctx_set_cost(ctx, 1, None))
            elif cost == "adcensus":
                _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
            for guide, entry, imgs, ch in (("gray", L.smx_ctx_stereo_pair, gray, 0), ("rgb", L.smx_ctx_stereo_pair_rgb, rgb, 3)):
                want = _ctx_want(orc, scene, cost, guide)
                for want_vol in (True, False):
                    rc, got = _ctx_pair(ctx, entry, imgs, ch, want_vol)
                    _lib.check(rc)
                    for k, name in names + ((("agg_l", "aggl"), ("agg_r", "aggr")) if want_vol else ()):
                        _eq(got[k], want[name], f"ctx cost {cost} guide {guide} {name} (volumes {want_vol})")
                    if want_vol:
                        _eq(got["cost_l"], scene["cost"][cost][0], f"ctx cost_l {cost}")
        # the later stages, against the chain
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, RATIO))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk())))
        want = chain(orc, scene["Il"], *scene["agg"][("adcensus", "rgb")])
        rc, got = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, rgb, 3, False)
        _lib.check(rc)
        _check_ctx_stages(ctx, got, want, "ctx stages")
        _lib.check(L.smx_ctx_set_subpixel(ctx, 0))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, 0.0))
        _lib.check(L.smx_ctx_set_speckle(ctx, None))
        # the refusals at the pair call
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, rgb, 3, False)
        assert rc == -1 and b"colour guidance" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_guidance(ctx, 0))
        _lib.check(L.smx_ctx_set_aggregation(ctx, 1, None))
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        assert rc == -1 and b"semi-global" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, 0, None))
        # off again: the oracle's pair
        _lib.check(L.smx_ctx_set_adcensus(ctx, None))
        _lib.check(L.smx_ctx_set_cross(ctx, None))
        rc, again = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False, mean=True)
        _lib.check(rc)
        for k, name in names:
            _eq(again[k], plain[name], "off again " + name)
    finally:
        L.smx_destroy(ctx)


@pytest.mark.parametrize("guide", ["gray", "rgb"])
@pytest.mark.parametrize("cost", [None, "adcensus"])
def test_context_chunks_do_not_change_a_bit(orc, scene, cost, guide):
    """The context's chunk loop under smx_set_max_slices_per_launch: 5 gives chunks of 5, 5, 5 and a ragged last one of a single
    slice, 16 one chunk, 1 every slice alone.  With the volumes the chunks go view by view into the whole volumes at their
    slice offsets; without them in the pair form from the chunk buffer.  Everything against the numpy references."""
    L = smx.lib()
    want = _ctx_want(orc, scene, cost, guide)
    entry, imgs, ch = (L.smx_ctx_stereo_pair, (scene["Il"], scene["Ir"]), 0) if guide == "gray" else \
                      (L.smx_ctx_stereo_pair_rgb, scene["rgb"], 3)
    ctx = _ctx_create()
    try:
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(_p(**PIPE_PARAMS))))
        if cost == "adcensus":
            _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
        for k in (1, 5, 16):
            for want_vol in (True, False):
                got = _bounded_pair(k, ctx, entry, imgs, ch, want_vol)
                for key, name in CTX_NAMES + (CTX_VOLUMES if want_vol else ()):
                    _eq(got[key], want[name], f"ctx cost {cost} guide {guide}, at most {k} slices, volumes {want_vol}: {name}")
    finally:
        L.smx_destroy(ctx)


def test_context_chunks_carry_the_states_of_the_later_stages(orc, scene):
    """Chunks of 5, 5, 5, 1 with sub-pixel, uniqueness and speckle removal on: the nbr / uq states accumulate across the
    context's chunks.  Against the chain that test_context compares with."""
    L = smx.lib()
    want = chain(orc, scene["Il"], *scene["agg"][("adcensus", "rgb")])
    ctx = _ctx_create()
    try:
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(_p(**PIPE_PARAMS))))
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, RATIO))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk())))
        for want_vol in (False, True):
            got = _bounded_pair(5, ctx, L.smx_ctx_stereo_pair_rgb, scene["rgb"], 3, want_vol)
            _check_ctx_stages(ctx, got, want, f"ctx stages in chunks of 5 (volumes {want_vol})")
            if want_vol:
                _eq(got["agg_l"], want["aggl"], "ctx stages in chunks of 5 aggl")
                _eq(got["agg_r"], want["aggr"], "ctx stages in chunks of 5 aggr")
    finally:
        L.smx_destroy(ctx)
