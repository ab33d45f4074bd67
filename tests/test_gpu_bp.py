"""Hierarchical belief propagation on the GPU (smx_dev_bp_wta_pair, smx_bp_aggregate, PairPipeline(aggregation="bp"), the
context entry), bit for bit against the numpy reference of tests/bp_ref.py.  Every device call hands its buffers over inside
guard bands (tests/guarded.py) with the workspace poisoned and off its alignment, so each case checks the memory contract too.

Run on the GPU box:  python -m pytest tests -m gpu -q -k bp
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import bp_ref as ref
import census_ref
import speckle_ref
import subpix_ref
import uniq_ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

# the smallest shapes at which each mechanism can go wrong: a single pixel; no neighbour in a direction; more rows (columns)
# than a block of senders; a lane boundary of the scan and padded labels; VPL 2 with odd pyramid sizes at every level; the
# VPL of the KITTI label count (192: lanes past the padded range); VPL 4
SHAPES = [(1, 1, 1), (1, 7, 2), (7, 1, 3), (5, 40, 9), (40, 5, 9), (65, 3, 63), (64, 4, 64), (63, 5, 65), (129, 70, 70),
          (130, 9, 192), (33, 6, 256)]
PENALTIES = [(20, 60), (0, 0), (7, 7), (1, 4095), (4095, 4095)]


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


def _p(step=20, trunc=60, iterations=5, levels=4, data_scale=1.0):
    p = _lib.BpParams()
    p.step, p.trunc, p.iterations, p.levels, p.data_scale = step, trunc, iterations, levels, data_scale
    return p


def _want(c, p):
    return ref.outputs(c, p.step, p.trunc, p.iterations, p.levels, p.data_scale)


class Call:
    """The buffers of one smx_dev_bp_wta_pair call, every one guarded; cost_l / cost_r: (D, h, w) float32 or None."""

    def __init__(self, cost_l, cost_r, levels=4, misalign=13, slots=None):
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
        self.uq = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.ws_bytes = smx.lib().smx_bp_workspace_bytes(w, h, D, levels, self.nviews)
        assert self.ws_bytes > 0
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)
        self.ws.view.fill_(0xC3)                                  # poison: the call may rely on nothing in here
        self.outs = ((self.keys, "keys"), (self.agg, "agg"), (self.nbr, "nbr"), (self.uq, "uq"))

    def run(self, p, ws_bytes=None, agg=True, nbr=True, uq=True):
        import torch
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda g: None if g is None else g.ptr
        return smx.lib().smx_dev_bp_wta_pair(C.byref(p), ptr(self.inp[0]), ptr(self.inp[1]), self.w, self.h, self.D,
                                              self.keys.ptr, self.agg.ptr if agg else None, self.nbr.ptr if nbr else None,
                                              self.uq.ptr if uq else None, self.ws.ptr,
                                              self.ws_bytes if ws_bytes is None else ws_bytes, st)

    def check_memory(self):
        for g, name in self.outs + ((self.ws, "ws"),):
            g.check("d_" + name)
        for g in self.inp:
            if g is not None:
                g.check_unchanged("d_cost")

    def check_against(self, p, label="", skip=()):
        """Run, then every output of every view equals the reference's, and nothing else was touched."""
        _lib.check(self.run(p, **{k: False for k in skip}))
        self.check_memory()
        got = {name: g.numpy() for g, name in self.outs}
        slot = 0
        for c in self.costs:
            if c is None:
                continue
            want = _want(c, p)
            for name in ("agg", "keys", "nbr", "uq"):
                if name not in skip:
                    _eq(got[name][slot], want[name], f"{label} {name}[{slot}]")
            slot += 1


def _costs(seed, D, h, w, hi):
    return np.random.default_rng(seed).integers(0, hi + 1, (D, h, w)).astype(np.float32)


@pytest.mark.parametrize("levels,iterations", [(1, 1), (1, 5), (4, 1), (4, 5)])
@pytest.mark.parametrize("w,h,D", SHAPES)
def test_against_the_reference(w, h, D, levels, iterations):
    for hi in (62, 255):
        call = Call(_costs(w * 1000 + D + hi, D, h, w, hi), _costs(h * 1000 + D + hi + 1, D, h, w, hi), levels=levels)
        for step, trunc in PENALTIES:
            call.ws.view.fill_(0xC3)
            call.check_against(_p(step, trunc, iterations, levels), f"{w}x{h}x{D} costs 0..{hi} V {step},{trunc}")


def test_data_scale_and_special_values_go_through_the_clamp():
    w, h, D = 21, 5, 10
    specials = np.array([-1, -0.0, 0.0, 0.5, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40, 0.124,
                         0.125, 15.9], np.float32)
    rng = np.random.default_rng(9)
    cost = specials[rng.integers(0, specials.size, (D, h, w))]
    odd_nan = np.array([0xFFC00001, 0x7F800001], np.uint32).view(np.float32)         # a negative NaN, a signalling one
    cost[0, 0, :2] = odd_nan
    call = Call(cost, cost[:, ::-1].copy())
    call.check_against(_p(), "special values")
    call.check_against(_p(data_scale=8.0), "special values, scale 8")
    small = (rng.random((D, h, w)) * 2.5).astype(np.float32)
    Call(small, small[:, :, ::-1].copy()).check_against(_p(data_scale=16.0), "costs in [0, 2.5], scale 16")


def test_tie_rule():
    w, h, D = 37, 6, 67
    const = np.full((D, h, w), 23, np.float32)
    rng = np.random.default_rng(5)
    # exactly two minima of the cost per pixel, and step = trunc = 0 so that S = C keeps them both
    two = rng.integers(10, 200, (D, h, w)).astype(np.float32)
    za = rng.integers(0, D, (h, w))
    zb = (za + rng.integers(1, D, (h, w))) % D
    np.put_along_axis(two, za[None], 3, axis=0)
    np.put_along_axis(two, zb[None], 3, axis=0)
    call = Call(const, two)
    call.check_against(_p(), "tie, default penalties")
    call.check_against(_p(0, 0), "tie, no penalties")
    keys = call.keys.numpy()
    assert (keys[0] == smx.lib().smx_pack_key(23.0, D - 1)).all()                         # constant: the LAST slice
    assert ((0xFFFFFFFF - (keys[1] & 0xFFFFFFFF)) == np.maximum(za, zb)).all()           # two minima: the later one


@pytest.mark.parametrize("left", [True, False])
def test_one_view_forms_leave_the_other_view_alone(left):
    w, h, D = 19, 6, 66
    cost = _costs(11, D, h, w, 255)
    call = Call(cost if left else None, None if left else cost, slots=2)
    call.check_against(_p(), "one view")
    for g, name in call.outs:
        tail = g.bytes[g.nbytes // 2:]
        assert bool((tail == g.fill).all()), f"{name}: the second view's half was written by a one-view call"


@pytest.mark.parametrize("misalign", [0, 1, 255])
def test_workspace_alignment_and_optional_outputs(misalign):
    w, h, D = 70, 9, 130
    cl, cr = _costs(21, D, h, w, 62), _costs(22, D, h, w, 62)
    Call(cl, cr, misalign=misalign).check_against(_p(), f"misalign {misalign}")
    for absent in ("agg", "nbr", "uq"):
        call = Call(cl, cr, misalign=misalign)
        call.check_against(_p(), f"without {absent}", skip=(absent,))
        getattr(call, absent).check_untouched(f"d_{absent} (not requested)")


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    call = Call(_costs(31, 9, 5, 17, 62), _costs(32, 9, 5, 17, 62))
    call.ws.view.fill_(call.ws.fill)
    assert call.run(_p(), ws_bytes=call.ws_bytes - 1) == -3
    assert b"workspace" in smx.lib().smx_last_error()
    for g, name in call.outs + ((call.ws, "ws"),):
        g.check_untouched("d_" + name)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    import torch
    w, h, D = 129, 70, 70
    call = Call(_costs(41, D, h, w, 62), _costs(42, D, h, w, 255))
    p = _p()
    _lib.check(call.run(p))
    first = [g.numpy().copy() for g, _ in call.outs]
    call.ws.view.fill_(0x11)
    _lib.check(call.run(p))
    for a, (g, name) in zip(first, call.outs):
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
    for g, _ in call.outs:
        g.view.zero_()
    call.ws.view.fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, (g, name) in zip(first, call.outs):
        _eq(g.numpy(), a, "graph replay " + name)
    call.check_memory()


def test_host_pointer_entry():
    w, h, D = 45, 11, 20
    cost = _costs(51, D, h, w, 62)
    p = _p(7, 50, 3, 2)
    agg, best, disp = smx.bp_aggregate(cost, dmin=-19, params=p)
    want = _want(cost, p)
    _eq(agg, want["agg"], "agg")
    _eq(best, want["best"], "best")
    _eq(disp, (want["z"] - 19).astype(np.float32), "disp_map")
    assert smx.bp_aggregate(cost, want_agg=False)[0] is None


# ---------------------------------------------------------------------------------------------
# the pipeline and the context
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL = 129, 70, 16, -15
SPK = (30, 1.0)
RATIO = 0.15
#          name        census  subpixel  uniqueness  speckle
OPTIONS = [("subpixel", False, True, False, False), ("uniqueness", False, False, True, False),
           ("speckle", False, False, False, True), ("census", True, False, False, False), ("all", True, True, True, True)]


def _bp():
    # the reference's cost is 2.5 wide: the scale spreads it over the clamp's range.  Weak smoothing on purpose, so that the
    # later stages have something to remove (at the defaults the speckle filter changes nothing on this scene)
    return _p(4, 8, 2, 2, 16.0)


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


@pytest.fixture(scope="module")
def pair():
    return synth.gen_pair(W, H, D, 4711)


@pytest.fixture(scope="module")
def volumes(pair, orc):
    """bp_ref.outputs of both views for the reference's cost and the census cost, computed once"""
    Il, Ir = pair
    p = _bp()
    cost = {False: (orc.cost_volume(Il, Ir, D, DMINL), orc.cost_volume(Ir, Il, D, 0)),
            True: (census_ref.census_cost(Il, Ir, D, DMINL), census_ref.census_cost(Ir, Il, D, 0))}
    return {c: (_want(cl, p), _want(cr, p)) for c, (cl, cr) in cost.items()}


def _chain(orc, sl, sr, subpixel, uniqueness, speckle):
    """cost -> bp_ref -> the existing finish references"""
    r = {"aggl": sl["agg"], "aggr": sr["agg"], "bestl": sl["best"], "bestr": sr["best"]}
    r["dmapl"] = (DMINL + sl["z"]).astype(np.float32)
    r["dmapr"] = sr["z"].astype(np.float32)
    r["occlusion"] = kept = orc.detect_occlusion(r["dmapl"], r["dmapr"], DMINL - 100)
    if uniqueness:
        has = np.ones((H, W), bool)
        r["unique"], r["margin"] = uniq_ref.apply(kept, has, sl["best"], sl["uq"][0], RATIO, DMINL, DMINL - 100)
        kept = r["unique"]
    if speckle:
        r["despeckled"] = kept = speckle_ref.speckle_filter(kept, DMINL, DMINL - 100, *SPK)
    r["filled"] = orc.fill_occlusion(kept, DMINL)
    if subpixel:
        mode = subpix_ref.MODES["parabola"]
        r["subpixl"], r["subpix_filled"] = subpix_ref.maps(mode, sl["z"], sl["best"], sl["nbr"][0], sl["nbr"][1], r["dmapl"], kept,
                                                           r["filled"], DMINL)
        r["subpixr"], _ = subpix_ref.maps(mode, sr["z"], sr["best"], sr["nbr"][0], sr["nbr"][1], r["dmapr"])
    return r


@pytest.mark.parametrize("name,census,subpixel,uniqueness,speckle", OPTIONS)
def test_pipeline(pair, volumes, orc, name, census, subpixel, uniqueness, speckle):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = pair
    want = _chain(orc, *volumes[census], subpixel, uniqueness, speckle)
    pipe = PairPipeline(W, H, D, dminl=DMINL, aggregation="bp", bp_params=_bp(), want_agg=True, cost="census" if census else None,
                        subpixel="parabola" if subpixel else None, uniqueness=RATIO if uniqueness else None,
                        speckle=_spk() if speckle else None)
    pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
    assert pipe.bp_ws is not None and pipe.bp_cost is not None and pipe.sgm_ws is None and pipe.ws_bytes == 0
    got = pipe.results()
    for k in want:
        _eq(got[k], want[k], f"{name}: {k}")
    if uniqueness:
        assert np.any(want["unique"] != want["occlusion"])
    if speckle:
        assert np.any(want["despeckled"] != (want["unique"] if uniqueness else want["occlusion"]))


def test_pipeline_defaults_and_refusals(pair):
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    pipe = PairPipeline(W, H, D, aggregation="bp")
    q = pipe.bp_params
    assert (q.step, q.trunc, q.iterations, q.levels, q.data_scale) == (20, 60, 5, 4, 1.0)
    none = PairPipeline(W, H, D)
    assert none.bp_ws is None and none.bp_cost is None and none.bp_params is None and none.bp_ws_bytes == 0
    for kw in (dict(aggregation="bp", s_begin=0, s_end=D // 2), dict(aggregation="bp", max_ws_bytes=1 << 20),
               dict(aggregation="bp", guidance="rgb"), dict(aggregation="bp", cross_scale=True),
               dict(aggregation="bp", permeability=True), dict(aggregation="sgm", bp_params=_bp()), dict(bp_params=_bp())):
        with pytest.raises(ValueError):
            PairPipeline(W, H, D, **kw)
    with pytest.raises(ValueError):
        PairPipeline(W, H, 257, aggregation="bp")
    with pytest.raises(ValueError, match="belief propagation"):
        ShardedPair(W, H, D, aggregation="bp")


def _ctx_pair(L, ctx, Il, Ir, want_agg=True, mean=False):
    n = W * H
    bufs = {k: np.empty((H, W), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if want_agg:
        bufs["agg_l"], bufs["agg_r"] = np.empty((D, H, W), np.float32), np.empty((D, H, W), np.float32)
    if mean:
        bufs["mean_l"] = np.empty(n, np.uint8)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    rc = L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, 0, C.byref(out))
    names = {"best_l": "bestl", "best_r": "bestr", "dmap_l": "dmapl", "dmap_r": "dmapr", "agg_l": "aggl", "agg_r": "aggr"}
    return rc, {names.get(k, k): v for k, v in bufs.items()}


def _held(L, ctx):
    nbytes = C.c_size_t()
    _lib.check(L.smx_ctx_bp_held(ctx, C.byref(nbytes)))
    return nbytes.value


@pytest.mark.parametrize("name,census,subpixel,uniqueness,speckle", OPTIONS)
def test_context(pair, volumes, orc, name, census, subpixel, uniqueness, speckle):
    Il, Ir = pair
    want = _chain(orc, *volumes[census], subpixel, uniqueness, speckle)
    L = smx.lib()
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), W, H, D, C.byref(ctx)))
    try:
        _lib.check(L.smx_ctx_set_bp(ctx, C.byref(_bp())))
        _lib.check(L.smx_ctx_set_cost(ctx, 1 if census else 0, None))
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1 if subpixel else 0))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, RATIO if uniqueness else 0.0))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk()) if speckle else None))
        assert _held(L, ctx) == 0
        rc, got = _ctx_pair(L, ctx, Il, Ir)
        _lib.check(rc)
        assert _held(L, ctx) == L.smx_bp_workspace_bytes(W, H, D, _bp().levels, 2)
        plane = lambda: np.empty((H, W), np.float32)
        if subpixel:
            got["subpixl"], got["subpixr"], got["subpix_filled"] = plane(), plane(), plane()
            _lib.check(L.smx_ctx_subpixel_maps(ctx, *(got[k].ctypes.data for k in ("subpixl", "subpixr", "subpix_filled"))))
        if uniqueness:
            got["unique"], got["margin"] = plane(), plane()
            _lib.check(L.smx_ctx_uniqueness_map(ctx, got["unique"].ctypes.data, got["margin"].ctypes.data))
        if speckle:
            got["despeckled"] = plane()
            _lib.check(L.smx_ctx_speckle_map(ctx, got["despeckled"].ctypes.data))
        for k in want:
            _eq(got[k], want[k], f"ctx {name}: {k}")
    finally:
        L.smx_destroy(ctx)


def test_context_refusals_and_off_by_default(pair):
    Il, Ir = pair
    L = smx.lib()
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), W, H, D, C.byref(ctx)))
    try:
        for bad in (_p(step=4096), _p(trunc=-1), _p(iterations=65), _p(levels=0), _p(levels=9), _p(data_scale=0.0),
                    _p(data_scale=float("nan"))):
            assert L.smx_ctx_set_bp(ctx, C.byref(bad)) == -1 and b"smx_ctx_set_bp" in L.smx_last_error()
        # never on, or on and off again before the first pair: nothing is held
        rc, plain = _ctx_pair(L, ctx, Il, Ir, want_agg=False)
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_bp(ctx, C.byref(_bp())))
        _lib.check(L.smx_ctx_set_bp(ctx, None))
        rc, again = _ctx_pair(L, ctx, Il, Ir, want_agg=False)
        _lib.check(rc)
        assert _held(L, ctx) == 0
        for k in plain:
            _eq(again[k], plain[k], "off again: " + k)
        _lib.check(L.smx_ctx_set_bp(ctx, C.byref(_bp())))
        assert _ctx_pair(L, ctx, Il, Ir, mean=True)[0] == -1 and b"mean" in L.smx_last_error()
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, 0) == -1
        assert b"smx_ctx_set_bp" in L.smx_last_error()
        xp, so, cs, pe, pm = (smx.default_cross_params(), smx.default_scanline_params(), smx.default_cscale_params(),
                              smx.default_perm_params(), smx.default_pm_params())
        conflicts = [(lambda: L.smx_ctx_set_aggregation(ctx, 1, None), lambda: L.smx_ctx_set_aggregation(ctx, 0, None), b"semi-global"),
                     (lambda: L.smx_ctx_set_cross(ctx, C.byref(xp)), lambda: L.smx_ctx_set_cross(ctx, None), b"cross-based"),
                     (lambda: L.smx_ctx_set_scanline(ctx, C.byref(so)), lambda: L.smx_ctx_set_scanline(ctx, None), b"scan-line"),
                     (lambda: L.smx_ctx_set_cross_scale(ctx, C.byref(cs)), lambda: L.smx_ctx_set_cross_scale(ctx, None), b"cross-scale"),
                     (lambda: L.smx_ctx_set_permeability(ctx, C.byref(pe)), lambda: L.smx_ctx_set_permeability(ctx, None), b"permeability"),
                     (lambda: L.smx_ctx_set_patchmatch(ctx, C.byref(pm)), lambda: L.smx_ctx_set_patchmatch(ctx, None), b"PatchMatch")]
        for on, off, word in conflicts:
            _lib.check(on())
            assert _ctx_pair(L, ctx, Il, Ir)[0] == -1
            err = L.smx_last_error()
            assert b"smx_ctx_set_bp" in err and word in err, err
            _lib.check(off())
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        rgb = np.repeat(Il[:, :, None], 3, axis=2).copy()
        out = _lib.PairOut()
        assert L.smx_ctx_stereo_pair_rgb(ctx, rgb.ctypes.data, rgb.ctypes.data, 3, DMINL, 0, C.byref(out)) == -1
        assert b"colour guidance" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_guidance(ctx, 0))
        assert _held(L, ctx) == 0                    # (every refusal came before anything was reserved)
        _lib.check(_ctx_pair(L, ctx, Il, Ir)[0])
    finally:
        L.smx_destroy(ctx)
    big = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), 16, 8, 257, C.byref(big)))
    try:
        _lib.check(L.smx_ctx_set_bp(big, None))
        _lib.check(L.smx_ctx_set_bp(big, C.byref(_bp())))
        a = np.zeros((8, 16), np.uint8)
        out = _lib.PairOut()
        assert L.smx_ctx_stereo_pair(big, a.ctypes.data, a.ctypes.data, -256, 0, C.byref(out)) == -1
        assert b"size_d" in L.smx_last_error()
    finally:
        L.smx_destroy(big)
