"""The scan-line optimiser with colour-adaptive penalties on the GPU (smx_dev_scanline_wta_pair, smx_scanline_optimize,
stages.scanline_optimize), bit for bit against the numpy reference of tests/scanline_ref.py.  Every device call hands its
buffers over inside guard bands (tests/guarded.py) with the workspace poisoned and off its alignment, so each case checks the
memory contract too.

Run on the GPU box:  python -m pytest tests -m gpu -q -k scanline
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import scanline_ref as ref
import sgm_ref
import uniq_ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 63, 64, 65, 129)
HEIGHTS = (1, 2, 5, 70)
SIZES_D = (1, 2, 63, 64, 65, 128, 129, 192, 256)


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


def _p(p1=127, p2=382, tau_so=15, paths=4):
    p = _lib.ScanlineParams()
    p.p1, p.p2, p.tau_so, p.paths = p1, p2, tau_so, paths
    return p


def _kw(p):
    return dict(p1=p.p1, p2=p.p2, tau_so=p.tau_so, paths=p.paths)


def _costs(seed, D, h, w, hi=255):
    return np.random.default_rng(seed).integers(0, hi + 1, (D, h, w)).astype(np.float32)


def _guide(kind, seed, h, w, ch):
    """constant: no edge anywhere; checker: every step an edge of 40; textured: steps around tau_so = 15, so both answers occur"""
    rng = np.random.default_rng(seed)
    if kind == "constant":
        g = np.full((h, w, ch), 77, np.uint8)
    elif kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.repeat((100 + 40 * ((yy + xx) & 1)).astype(np.uint8)[:, :, None], ch, axis=2)
    else:
        g = (100 + rng.integers(0, 26, (h, w, ch))).astype(np.uint8)
    if ch == 4:
        g[:, :, 3] = rng.integers(0, 256, (h, w))           # a fourth byte is ignored
    return np.ascontiguousarray(g[:, :, 0] if ch == 1 else g)


def _uq_ref(S):
    """The planes sec, rest, last of one run over all slices (tests/uniq_ref.py), for integer S."""
    _, _, sec, rest, last, _ = uniq_ref.second_best(S.astype(np.float32))
    return np.stack((sec, rest, last)).astype(np.float32)


class Call:
    """The buffers of one smx_dev_scanline_wta_pair call, every one guarded; cost_l / cost_r: (D, h, w) float32 or None; the
    guides (h, w) or (h, w, channels) uint8, always both."""

    def __init__(self, guide_l, guide_r, cost_l, cost_r, dminl, dminr, misalign=13, slots=None):
        self.costs, self.guides, self.dmin = (cost_l, cost_r), (guide_l, guide_r), (dminl, dminr)
        D, h, w = (cost_l if cost_l is not None else cost_r).shape
        self.D, self.h, self.w, self.n = D, h, w, w * h
        self.ch = 1 if guide_l.ndim == 2 else guide_l.shape[2]
        self.nviews = (cost_l is not None) + (cost_r is not None)
        slots = self.nviews if slots is None else slots
        n = self.n
        self.inp = [None if c is None else Guarded(c.nbytes, np.float32, c.shape, plane=n).load(c) for c in self.costs]
        self.gd = [Guarded(g.nbytes, np.uint8, g.shape, plane=n).load(g) for g in self.guides]
        self.keys = Guarded(slots * n * 8, np.int64, (slots, h, w), plane=n)
        self.agg = Guarded(slots * D * n * 4, np.float32, (slots, D, h, w), plane=n)
        self.nbr = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.uq = Guarded(slots * 3 * n * 4, np.float32, (slots, 3, h, w), plane=n)
        self.ws_bytes = smx.lib().smx_scanline_workspace_bytes(w, h, D, self.nviews)
        assert self.ws_bytes > 0
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)
        self.ws.view.fill_(0xFF)                                  # poison: every edge flag set, every cost and sum at its top

    def run(self, p, ws_bytes=None, agg=True, nbr=True, uq=True):
        import torch
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ptr = lambda g: None if g is None else g.ptr
        return smx.lib().smx_dev_scanline_wta_pair(
            C.byref(p), self.gd[0].ptr, self.gd[1].ptr, self.ch, ptr(self.inp[0]), ptr(self.inp[1]), self.w, self.h, self.D,
            self.dmin[0], self.dmin[1], self.keys.ptr, self.agg.ptr if agg else None, self.nbr.ptr if nbr else None,
            self.uq.ptr if uq else None, self.ws.ptr, self.ws_bytes if ws_bytes is None else ws_bytes, st)

    def outputs(self):
        return self.keys, self.agg, self.nbr, self.uq

    def check_memory(self):
        for g, name in ((self.keys, "d_keys"), (self.agg, "d_agg"), (self.nbr, "d_nbr"), (self.uq, "d_uq"), (self.ws, "d_ws")):
            g.check(name)
        for g in self.inp:
            if g is not None:
                g.check_unchanged("d_cost")
        for g in self.gd:
            g.check_unchanged("d_guide")

    def want(self, p):
        """per given view: the reference's outputs"""
        out = []
        for v, c in enumerate(self.costs):
            if c is not None:
                out.append(ref.outputs(self.guides[v], self.guides[1 - v], c, self.dmin[v], **_kw(p)))
        return out

    def check_against(self, p, label="", want=None):
        """Run, then every output of every view equals the reference's, and nothing else was touched."""
        _lib.check(self.run(p))
        self.check_memory()
        keys, agg, nbr, uq = (g.numpy() for g in self.outputs())
        for slot, w in enumerate(self.want(p) if want is None else want):
            _eq(agg[slot], w["agg"], f"{label} agg[{slot}]")
            _eq(keys[slot], w["keys"], f"{label} keys[{slot}]")
            _eq(nbr[slot], w["nbr"], f"{label} nbr[{slot}]")
            _eq(uq[slot], _uq_ref(w["S"]), f"{label} uq[{slot}]")


def _dmins(w, D):
    """(dminl, dminr): the reference's convention, zero, every partner outside on either side, ranges that straddle a border"""
    return [(-(D - 1), 0), (0, 0), (w, -w - D), (-w - D, w), (-(D // 2) - 1, w - D // 2 - 1), (w - 1, -D)]


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_sizes(w, h):
    """Every width and height of the list (3 x 70: every diagonal wraps many times), the label counts in turn, eight paths
    and four, every kind of guide, every dmin case."""
    i = WIDTHS.index(w) * len(HEIGHTS) + HEIGHTS.index(h)
    D = SIZES_D[i % len(SIZES_D)]
    kinds = ("textured", "checker", "constant")
    for j, (dl, dr) in enumerate(_dmins(w, D)):
        ch = (1, 3, 4)[(i + j) % 3]
        gl, gr = _guide(kinds[j % 3], 10 * i + j, h, w, ch), _guide(kinds[(j + 1) % 3 if j else 0], 10 * i + j + 2, h, w, ch)
        call = Call(gl, gr, _costs(1000 * i + j, D, h, w), _costs(2000 * i + j, D, h, w, 62), dl, dr)
        call.check_against(_p(127, 382, 15, 8 if j & 1 else 4), f"{w}x{h}x{D} dmin {dl},{dr} ch {ch}")


@pytest.mark.parametrize("D", SIZES_D)
def test_label_counts(D):
    """Every VPL, idle lanes and the padding, on a shape with more than one block whose diagonals wrap, textured guides."""
    w, h = 21, 9
    gl, gr = _guide("textured", D, h, w, 3), _guide("textured", D + 1, h, w, 3)
    call = Call(gl, gr, _costs(D, D, h, w), _costs(D + 7, D, h, w), -(D - 1), 0)
    for paths in (4, 8):
        call.check_against(_p(20, 200, 15, paths), f"D {D} paths {paths}")
    Call(gl, gr, _costs(D, D, h, w), _costs(D + 7, D, h, w), -(D // 2), -3).check_against(_p(127, 382, 12, 8), f"D {D} straddle")


@pytest.mark.parametrize("paths", [4, 8])
def test_tau_and_penalties(paths):
    w, h, D = 65, 5, 65
    gl, gr = _guide("textured", 3, h, w, 3), _guide("textured", 4, h, w, 3)
    call = Call(gl, gr, _costs(5, D, h, w), _costs(6, D, h, w), -(D - 1), 0)
    for tau in (1, 15, 256):
        for p1, p2 in ((0, 0), (3, 4095), (127, 382)):
            call.check_against(_p(p1, p2, tau, paths), f"tau {tau} p {p1},{p2}")


@pytest.mark.parametrize("paths", [4, 8])
def test_tau_256_equals_sgm_on_the_device(paths):
    import torch
    w, h, D = 129, 5, 129
    gl, gr = _guide("checker", 1, h, w, 3), _guide("textured", 2, h, w, 3)
    cl, cr = _costs(7, D, h, w), _costs(8, D, h, w, 62)
    call = Call(gl, gr, cl, cr, -(D - 1), 0)
    _lib.check(call.run(_p(10, 120, 256, paths)))
    n = w * h
    L = smx.lib()
    dev = lambda a: torch.from_numpy(a).cuda()
    tl, tr = dev(cl), dev(cr)
    keys = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    agg = torch.empty((2, D, h, w), dtype=torch.float32, device="cuda")
    nbr, uq = (torch.empty((2, 3, h, w), dtype=torch.float32, device="cuda") for _ in range(2))
    wsb = L.smx_sgm_workspace_bytes(w, h, D, 2)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    sp = _lib.SgmParams()
    sp.p1, sp.p2, sp.paths = 10, 120, paths
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.smx_dev_sgm_wta_pair_uq(C.byref(sp), tl.data_ptr(), tr.data_ptr(), w, h, D, keys.data_ptr(), agg.data_ptr(),
                                         nbr.data_ptr(), uq.data_ptr(), ws.data_ptr(), wsb, st))
    torch.cuda.synchronize()
    for g, t, name in zip(call.outputs(), (keys, agg, nbr, uq), ("keys", "agg", "nbr", "uq")):
        _eq(g.numpy(), t.cpu().numpy(), "against smx_dev_sgm_wta_pair: " + name)
    _eq(call.agg.numpy()[0], sgm_ref.outputs(cl, 10, 120, paths)["agg"], "against sgm_ref")
    assert n > 0


def test_equality_with_tau_is_an_edge():
    """One step of exactly tau_so and one of tau_so - 1 in each view, away from everything else."""
    w, h, D = 20, 3, 4
    gl = np.full((h, w), 50, np.uint8); gr = gl.copy()
    gl[:, 6:] += 15; gl[:, 12:] += 14
    gr[:, 8:] += 14; gr[:, 14:] += 15
    call = Call(gl, gr, _costs(1, D, h, w, 62), _costs(2, D, h, w, 62), 0, -3)
    p = _p(40, 400, 15, 8)
    call.check_against(p, "equality")
    assert ref.edges(gl, 1, 0, 15)[:, 6].all() and not ref.edges(gl, 1, 0, 15)[:, 12].any()
    other = [ref.outputs(gl, gr, c, d, p1=40, p2=400, tau_so=16, paths=8)["S"] for c, d in zip(call.costs, call.dmin)]
    assert all(np.any(o != w_["S"]) for o, w_ in zip(other, call.want(p)))          # the step of 15 counts at 15, not at 16


def test_special_values_go_through_the_clamp():
    w, h, D = 21, 5, 10
    specials = np.array([-1, -0.0, 0.0, 0.5, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40],
                        np.float32)
    rng = np.random.default_rng(9)
    cost = specials[rng.integers(0, specials.size, (D, h, w))]
    cost[0, 0, :2] = np.array([0xFFC00001, 0x7F800001], np.uint32).view(np.float32)   # a negative NaN, a signalling one
    gl, gr = _guide("textured", 5, h, w, 4), _guide("textured", 6, h, w, 4)
    Call(gl, gr, cost, cost[:, ::-1].copy(), -4, -5).check_against(_p(paths=8), "special values")


@pytest.mark.parametrize("left", [True, False])
def test_one_view_forms_leave_the_other_view_alone(left):
    w, h, D = 19, 6, 66
    cost = _costs(11, D, h, w)
    gl, gr = _guide("textured", 7, h, w, 3), _guide("checker", 8, h, w, 3)
    call = Call(gl, gr, cost if left else None, None if left else cost, -9, -40, slots=2)
    call.check_against(_p(paths=8), "one view")
    for g, name in ((call.keys, "keys"), (call.agg, "agg"), (call.nbr, "nbr"), (call.uq, "uq")):
        tail = g.bytes[g.nbytes // 2:]
        assert bool((tail == g.fill).all()), f"{name}: the second view's half was written by a one-view call"


@pytest.mark.parametrize("misalign", [0, 1, 255])
def test_workspace_alignment_and_optional_outputs(misalign):
    w, h, D = 70, 9, 130
    cl, cr = _costs(21, D, h, w, 62), _costs(22, D, h, w, 62)
    gl, gr = _guide("textured", 9, h, w, 1), _guide("textured", 10, h, w, 1)
    p = _p()
    first = Call(gl, gr, cl, cr, -(D - 1), 0, misalign=misalign)
    want = first.want(p)
    first.check_against(p, f"misalign {misalign}", want)
    for on in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        call = Call(gl, gr, cl, cr, -(D - 1), 0, misalign=misalign)
        _lib.check(call.run(p, agg=on[0], nbr=on[1], uq=on[2]))
        call.check_memory()
        for g, name, there, key in zip((call.agg, call.nbr, call.uq), ("d_agg", "d_nbr", "d_uq"), on, ("agg", "nbr", None)):
            if not there:
                g.check_untouched(name + " (not requested)")
            elif key:
                _eq(g.numpy()[1], want[1][key], name)
            else:
                _eq(g.numpy()[1], _uq_ref(want[1]["S"]), name)
        _eq(call.keys.numpy()[1], want[1]["keys"], "keys")


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    w, h, D = 17, 5, 9
    g = _guide("textured", 1, h, w, 3)
    for cl, cr in ((_costs(31, D, h, w), _costs(32, D, h, w)), (_costs(31, D, h, w), None), (None, _costs(32, D, h, w))):
        call = Call(g, g, cl, cr, 0, 0)
        call.ws.view.fill_(call.ws.fill)
        assert call.run(_p(), ws_bytes=call.ws_bytes - 1) == -3
        assert b"workspace" in smx.lib().smx_last_error()
        for b, name in ((call.keys, "d_keys"), (call.agg, "d_agg"), (call.nbr, "d_nbr"), (call.uq, "d_uq"), (call.ws, "d_ws")):
            b.check_untouched(name)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    import torch
    w, h, D = 129, 70, 70
    gl, gr = _guide("textured", 11, h, w, 3), _guide("textured", 12, h, w, 3)
    call = Call(gl, gr, _costs(41, D, h, w, 62), _costs(42, D, h, w), -(D - 1), 0)
    p = _p(paths=8)
    call.check_against(p, "first run")
    names = ("keys", "agg", "nbr", "uq")
    first = [g.numpy().copy() for g in call.outputs()]
    call.ws.view.fill_(0x11)
    _lib.check(call.run(p))
    for a, g, name in zip(first, call.outputs(), names):
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
    for g in call.outputs():
        g.view.zero_()
    call.ws.view.fill_(0x77)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for a, g, name in zip(first, call.outputs(), names):
        _eq(g.numpy(), a, "graph replay " + name)
    call.check_memory()


def test_host_pointer_entry_and_stage():
    w, h, D = 45, 11, 20
    cost = _costs(51, D, h, w, 62)
    go, gx = _guide("textured", 13, h, w, 3), _guide("textured", 14, h, w, 3)
    p = _p(40, 400, 15, 8)
    agg, best, disp = smx.scanline_optimize(go, gx, cost, dmin=-7, params=p)
    want = ref.outputs(go, gx, cost, -7, **_kw(p))
    _eq(agg, want["agg"], "agg")
    _eq(best, want["best"], "best")
    _eq(disp, (want["z"] - 7).astype(np.float32), "disp_map")
    assert smx.scanline_optimize(go, gx, cost, want_agg=False)[0] is None
    d = smx.scanline_optimize(go, gx, cost)[2]                   # the defaults
    _eq(d, ref.outputs(go, gx, cost, 0)["z"].astype(np.float32), "defaults")


def test_the_thin_strip_survives_on_the_device():
    """The scene of tests/test_scanline_cpu.py through the kernels: adaptive penalties at 40 / 400 get every pixel, the
    constant ones (tau_so = 256) lose strip pixels."""
    gl, gr, cost, truth = ref.thin_scene()
    d = smx.scanline_optimize(gl, gr, cost, params=_p(40, 400, 15, 4), want_agg=False)[2]
    assert int((d != truth).sum()) == 0
    d = smx.scanline_optimize(gl, gr, cost, params=_p(40, 400, 256, 4), want_agg=False)[2]
    assert int((d != truth).sum()) == 26


# ---------------------------------------------------------------------------------------------
# the pipeline and the context, on Tsukuba
# ---------------------------------------------------------------------------------------------
TD, TDMINL = 16, -15
CROSS = dict(l1=9, l2=4, tau1=20, tau2=6, iterations=1)       # (short arms, one iteration, four paths: the references stay quick;
SO = dict(p1=40, p2=400, tau_so=15, paths=4)                  # the device entry's own tests above run the eight)
MAPS = ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")
AGGS = ("scanline", "cross-scanline")


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _xp(**kw):
    p = smx.default_cross_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _maps_of(orc, so_l, so_r):
    """The volumes and the six planes behind the winners of both views' S"""
    want = {"aggl": so_l["agg"], "aggr": so_r["agg"], "bestl": so_l["best"], "bestr": so_r["best"],
            "dmapl": (TDMINL + so_l["z"]).astype(np.float32), "dmapr": so_r["z"].astype(np.float32)}
    want["occlusion"] = orc.detect_occlusion(want["dmapl"], want["dmapr"], TDMINL - 100)
    want["filled"] = orc.fill_occlusion(want["occlusion"], TDMINL)
    return want


@pytest.fixture(scope="module")
def tsukuba(orc, golden):
    """The colour pair, its gray images, the three costs of both views, and a cache of the chained references: per
    (aggregation, cost, guide, parameters) the outputs of both views, computed once and left unchanged."""
    import adcensus_ref
    import census_ref
    import cross_ref
    rgb = (np.ascontiguousarray(golden["tsukuba0"]), np.ascontiguousarray(golden["tsukuba1"]))
    Il, Ir = orc.gray(rgb[0]), orc.gray(rgb[1])
    cost = {None: (orc.cost_volume(Il, Ir, TD, TDMINL), orc.cost_volume(Ir, Il, TD, 0)),
            "census": (census_ref.census_cost(Il, Ir, TD, TDMINL), census_ref.census_cost(Ir, Il, TD, 0)),
            "adcensus": (adcensus_ref.gray_cost(Il, Ir, TD, TDMINL), adcensus_ref.gray_cost(Ir, Il, TD, 0))}
    guides = {"gray": (Il, Ir), "rgb": rgb}
    cache = {}

    def q_of(c, g, v):
        if ("q", c, g, v) not in cache:
            cache[("q", c, g, v)] = cross_ref.aggregate(guides[g][v], cost[c][v], **CROSS)
        return cache[("q", c, g, v)]

    def want(agg, c, g, **so):
        key = (agg, c, g, tuple(sorted(so.items())))
        if key not in cache:
            out = []
            for v, dmin in ((0, TDMINL), (1, 0)):
                vol = q_of(c, g, v) if agg == "cross-scanline" else cost[c][v]
                out.append(ref.outputs(guides[g][v], guides[g][1 - v], vol, dmin, **so))
            cache[key] = tuple(out)
        return cache[key]

    return dict(rgb=rgb, Il=Il, Ir=Ir, cost=cost, want=want, q_of=q_of, h=Il.shape[0], w=Il.shape[1])


def _pipe(ts, agg, guide, run=True, so=SO, **kw):
    from stereo_matching_cuda_amd.device import PairPipeline
    if agg in AGGS and so is not None:
        kw["scanline_params"] = _p(**so)
    if agg in ("cross", "cross-scanline"):
        kw["cross_params"] = _xp(**CROSS)
    pipe = PairPipeline(ts["w"], ts["h"], TD, dminl=TDMINL, aggregation=agg, **kw)
    if run:
        rgb = dict(rgb_l=_t(ts["rgb"][0]), rgb_r=_t(ts["rgb"][1])) if guide == "rgb" else {}
        pipe.run(_t(ts["Il"]), _t(ts["Ir"]), **rgb)
    return pipe


@pytest.mark.parametrize("cost", [None, "census", "adcensus"])
@pytest.mark.parametrize("agg", AGGS)
def test_pipeline_on_tsukuba(orc, tsukuba, agg, cost):
    """Both new aggregations with the three costs against the chained numpy references; the colour guide, and for one cost the
    gray one; the chain with its cross stage in chunks."""
    for guide, sif in (("rgb", None), ("rgb", 5)) + ((("gray", None),) if cost == "adcensus" else ()):
        if sif and agg == "scanline":
            continue
        sl, sr = tsukuba["want"](agg, cost, guide, **SO)
        want = _maps_of(orc, sl, sr)
        pipe = _pipe(tsukuba, agg, guide, cost=cost, want_agg=True, slices_in_flight=sif)
        assert pipe.so_ws is not None and pipe.so_cost is not None and pipe.ws_bytes == 0
        assert (pipe.cross_ws is not None) == (agg == "cross-scanline") and (pipe._so_chunk is not None) == bool(sif)
        got = pipe.results()
        for k in want:
            _eq(got[k], want[k], f"{agg} cost {cost} guide {guide} sif {sif} {k}")
        _eq(pipe.keys.cpu().numpy(), np.stack((sl["keys"], sr["keys"])), "keys")
        assert not got["meanl"].any() and not got["meanr"].any()
        assert len(np.unique(want["dmapl"])) > 3


def test_defaults_and_the_clamp_of_the_chain(orc, tsukuba):
    """scanline_params=None is the defaults; the chain's optimiser reads q without its fractional bits."""
    sl, sr = tsukuba["want"]("scanline", "adcensus", "rgb", **ref.DEFAULTS)
    pipe = _pipe(tsukuba, "scanline", "rgb", cost="adcensus", want_agg=True, so=ref.DEFAULTS)
    pipe2 = _pipe(tsukuba, "scanline", "rgb", run=False, cost="adcensus", so=None)
    assert pipe2.so_params.p1 == 127 and pipe2.so_params.paths == 4
    _eq(pipe.results()["aggl"], sl["agg"], "defaults aggl")
    q = tsukuba["q_of"]("adcensus", "rgb", 0)
    assert np.any(q != np.floor(q))
    cl = tsukuba["want"]("cross-scanline", "adcensus", "rgb", **SO)[0]
    _eq(ref.outputs(tsukuba["rgb"][0], tsukuba["rgb"][1], np.floor(q), TDMINL, **SO)["agg"], cl["agg"], "floor(q)")


def test_composition_with_uniqueness_speckle_vote_subpixel_and_weighted_median(orc, tsukuba):
    import cgf_ref
    import vote_ref
    spk = _lib.SpeckleParams()
    spk.max_size, spk.max_diff = 30, 1.0
    sl, sr = tsukuba["want"]("cross-scanline", "adcensus", "rgb", **SO)
    pipe = _pipe(tsukuba, "cross-scanline", "rgb", cost="adcensus", want_agg=True, slices_in_flight=6, speckle=spk, uniqueness=0.05,
                 vote=True, subpixel="parabola", wmf="occluded")
    got = pipe.results()
    _eq(got["aggl"], sl["agg"], "aggl")
    _eq(got["aggr"], sr["agg"], "aggr")
    st = cgf_ref.states(sl["agg"])
    _eq(pipe.uq.cpu().numpy()[0], st["uq"], "uq")
    _eq(pipe.nbr.cpu().numpy()[0], st["nbr"], "nbr")
    e = dict(dmapl=(TDMINL + sl["z"]).astype(np.float32), dmapr=sr["z"].astype(np.float32), grayl=tsukuba["Il"])
    # the stages behind the winners, each reference from the one before it
    import speckle_ref
    import subpix_ref
    import uniq_ref
    import wmf_ref
    occ = orc.detect_occlusion(e["dmapl"], e["dmapr"], TDMINL - 100)
    uni = uniq_ref.apply(occ, st["z"] >= 0, st["best"], st["uq"][0], np.float32(0.05), TDMINL, TDMINL - 100)[0]
    desp = speckle_ref.speckle_filter(uni, TDMINL, TDMINL - 100, 30, 1.0)
    voted = vote_ref.region_vote_guide(desp, tsukuba["rgb"][0], e["dmapr"], TDMINL, TD, int(pipe.params.d_lr))
    filled = orc.fill_occlusion(voted, TDMINL)
    _, sub_filled = subpix_ref.maps(subpix_ref.MODES["parabola"], st["z"], st["best"], st["nbr"][0], st["nbr"][1], e["dmapl"], desp,
                                    filled, TDMINL)
    refined = wmf_ref.weighted_median(tsukuba["Il"], filled, TDMINL, TD, desp)
    for k, w_ in (("occlusion", occ), ("unique", uni), ("despeckled", desp), ("voted", voted), ("filled", filled),
                  ("subpix_filled", sub_filled), ("refined", refined)):
        _eq(got[k], w_, k)
    assert np.any(uni != occ) and np.any(voted != desp) and np.any(refined != filled)


def test_pipeline_given_volumes_and_refusals(orc, tsukuba):
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    w, h = tsukuba["w"], tsukuba["h"]
    Il, Ir = _t(tsukuba["Il"]), _t(tsukuba["Ir"])
    cl, cr = tsukuba["cost"]["census"]
    pipe = _pipe(tsukuba, "scanline", "gray", run=False, want_agg=True)
    pipe.aggregate(Il, Ir, _t(cl), _t(cr))
    pipe.finish()
    _eq(pipe.results()["aggr"], tsukuba["want"]("scanline", "census", "gray", **SO)[1]["agg"], "given volumes aggr")
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, _t(cl))                                   # one volume alone
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=_t(tsukuba["rgb"][0]))              # one guide alone
    for agg in AGGS:
        with pytest.raises(ValueError):
            PairPipeline(w, h, TD, aggregation=agg, s_begin=0, s_end=TD // 2)
        with pytest.raises(ValueError):
            PairPipeline(w, h, TD, aggregation=agg, max_ws_bytes=1 << 20)
        with pytest.raises(ValueError):
            PairPipeline(w, h, 257, aggregation=agg)
        with pytest.raises(ValueError):
            PairPipeline(w, h, TD, aggregation=agg, guidance="rgb")
        with pytest.raises(ValueError, match="scan-line"):
            ShardedPair(w, h, TD, aggregation=agg)
        with pytest.raises(_lib.SmxError):
            PairPipeline(w, h, TD, dminl=TDMINL, aggregation=agg, scanline_params=_p(p1=11, p2=10)).run(Il, Ir)
    with pytest.raises(ValueError):
        PairPipeline(w, h, TD, aggregation="sgm", scanline_params=_p())
    with pytest.raises(ValueError):
        PairPipeline(w, h, TD, scanline_params=_p())
    # max_ws_bytes counts the volumes, the workspaces and the chain's chunk buffers
    need = 2 * TD * w * h * 4 + smx.lib().smx_scanline_workspace_bytes(w, h, TD, 2)
    PairPipeline(w, h, TD, aggregation="scanline", max_ws_bytes=need)
    with pytest.raises(ValueError):
        PairPipeline(w, h, TD, aggregation="scanline", max_ws_bytes=need - 1)
    with pytest.raises(ValueError):
        PairPipeline(w, h, TD, aggregation="cross-scanline", max_ws_bytes=need)
    small = PairPipeline(w, h, TD, aggregation="cross-scanline", max_ws_bytes=need + (24 << 20))      # (all 16 slices: 55 MiB)
    assert 1 <= small.slices_in_flight < TD and small._so_chunk is not None


@pytest.mark.parametrize("agg", [None, "sgm", "cross"])
def test_the_other_aggregations_give_the_bytes_they_gave(tsukuba, agg):
    """Compared within the run against a pipeline built without the new arguments; nothing of the optimiser is allocated."""
    from stereo_matching_cuda_amd.device import PairPipeline
    kw = dict(cost="census") if agg == "sgm" else {}
    a = PairPipeline(tsukuba["w"], tsukuba["h"], TD, dminl=TDMINL, aggregation=agg, scanline_params=None, want_agg=True, **kw)
    b = PairPipeline(tsukuba["w"], tsukuba["h"], TD, dminl=TDMINL, aggregation=agg, want_agg=True, **kw)
    assert a.so_ws is None and a.so_cost is None and a.so_params is None and a._so_chunk is None and a.so_ws_bytes == 0
    for p in (a, b):
        p.run(_t(tsukuba["Il"]), _t(tsukuba["Ir"]))
    ra, rb = a.results(), b.results()
    assert ra.keys() == rb.keys()
    for k in ra:
        _eq(ra[k], rb[k], k)
    _eq(a.keys.cpu().numpy(), b.keys.cpu().numpy(), "keys")
    assert a.ws_bytes == b.ws_bytes and a.slices_in_flight == b.slices_in_flight


def _ctx_pair(ctx, ts, entry, imgs, channels, want_vol, mean=False):
    h, w = ts["h"], ts["w"]
    bufs = {k: np.empty((h, w), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if want_vol:
        for k in ("agg_l", "agg_r"):
            bufs[k] = np.empty((TD, h, w), np.float32)
    if mean:
        bufs["mean_l"] = np.empty((h, w), np.uint8)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    args = (imgs[0].ctypes.data, imgs[1].ctypes.data) + ((channels,) if channels else ()) + (TDMINL, 0, C.byref(out))
    return entry(ctx, *args), bufs


CTX_NAMES = (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"), ("occlusion", "occlusion"),
             ("filled", "filled"), ("agg_l", "aggl"), ("agg_r", "aggr"))


def test_context(orc, tsukuba):
    """Off, on (alone and behind cross-based aggregation, gray and colour entry, with and without the volumes, a bounded
    chunk), the later stages behind it, its error cases, off again."""
    L = smx.lib()
    ts = tsukuba
    gray, rgb = (ts["Il"], ts["Ir"]), ts["rgb"]
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), ts["w"], ts["h"], TD, C.byref(ctx)))
    try:
        rc, off = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        plain = orc.stereo_pair(*gray, TD, dminl=TDMINL, dminr=0)
        for k, name in CTX_NAMES[:6]:
            _eq(off[k], plain[name], "off " + name)
        for bad in (dict(p1=11, p2=10), dict(p2=4096), dict(tau_so=0), dict(tau_so=257), dict(paths=6)):
            assert L.smx_ctx_set_scanline(ctx, C.byref(_p(**bad))) == -1
        _lib.check(L.smx_ctx_set_scanline(ctx, C.byref(_p(**SO))))
        assert L.smx_ctx_stereo_pair_async(ctx, gray[0].ctypes.data, gray[1].ctypes.data, TDMINL, 0) == -1
        assert b"smx_ctx_set_scanline" in L.smx_last_error()
        rc, _ = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair, gray, 0, False, mean=True)
        assert rc == -1 and b"mean" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
        for agg in AGGS:
            if agg == "cross-scanline":
                _lib.check(L.smx_ctx_set_cross(ctx, C.byref(_xp(**CROSS))))
            for guide, entry, imgs, ch in (("gray", L.smx_ctx_stereo_pair, gray, 0), ("rgb", L.smx_ctx_stereo_pair_rgb, rgb, 3)):
                sl, sr = ts["want"](agg, "adcensus", guide, **SO)
                want = _maps_of(orc, sl, sr)
                for want_vol, bound in ((True, 0), (False, 5)):
                    _lib.check(L.smx_set_max_slices_per_launch(bound))
                    try:
                        rc, got = _ctx_pair(ctx, ts, entry, imgs, ch, want_vol)
                    finally:
                        L.smx_set_max_slices_per_launch(0)
                    _lib.check(rc)
                    for k, name in CTX_NAMES if want_vol else CTX_NAMES[:6]:
                        _eq(got[k], want[name], f"ctx {agg} guide {guide} {name} (volumes {want_vol})")
        # the later stages behind the chain
        import cgf_ref
        import speckle_ref
        import uniq_ref
        spk = _lib.SpeckleParams()
        spk.max_size, spk.max_diff = 30, 1.0
        _lib.check(L.smx_ctx_set_uniqueness(ctx, 0.05))
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(spk)))
        _lib.check(L.smx_ctx_set_subpixel(ctx, 1))
        rc, got = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair_rgb, rgb, 3, False)
        _lib.check(rc)
        sl, sr = ts["want"]("cross-scanline", "adcensus", "rgb", **SO)
        st = cgf_ref.states(sl["agg"])
        occ = orc.detect_occlusion((TDMINL + sl["z"]).astype(np.float32), sr["z"].astype(np.float32), TDMINL - 100)
        uni = uniq_ref.apply(occ, st["z"] >= 0, st["best"], st["uq"][0], np.float32(0.05), TDMINL, TDMINL - 100)[0]
        desp = speckle_ref.speckle_filter(uni, TDMINL, TDMINL - 100, 30, 1.0)
        _eq(got["occlusion"], occ, "ctx stages occlusion")
        _eq(got["filled"], orc.fill_occlusion(desp, TDMINL), "ctx stages filled")
        m = np.empty((ts["h"], ts["w"]), np.float32)
        _lib.check(L.smx_ctx_uniqueness_map(ctx, m.ctypes.data, None))
        _eq(m, uni, "ctx stages unique")
        _lib.check(L.smx_ctx_speckle_map(ctx, m.ctypes.data))
        _eq(m, desp, "ctx stages despeckled")
        _lib.check(L.smx_ctx_subpixel_maps(ctx, m.ctypes.data, None, None))
        import subpix_ref
        _eq(m, subpix_ref.maps(subpix_ref.MODES["parabola"], st["z"], st["best"], st["nbr"][0], st["nbr"][1],
                               (TDMINL + sl["z"]).astype(np.float32))[0], "ctx stages subpixl")
        _lib.check(L.smx_ctx_set_uniqueness(ctx, 0.0))
        _lib.check(L.smx_ctx_set_speckle(ctx, None))
        _lib.check(L.smx_ctx_set_subpixel(ctx, 0))
        # the refusals at the pair call
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        rc, _ = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair_rgb, rgb, 3, False)
        assert rc == -1 and b"colour guidance" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_guidance(ctx, 0))
        _lib.check(L.smx_ctx_set_cross(ctx, None))
        _lib.check(L.smx_ctx_set_aggregation(ctx, 1, None))
        rc, _ = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair, gray, 0, False)
        assert rc == -1 and b"semi-global" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, 0, None))
        # off, and on again
        _lib.check(L.smx_ctx_set_adcensus(ctx, None))
        _lib.check(L.smx_ctx_set_scanline(ctx, None))
        rc, again = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair, gray, 0, False, mean=True)
        _lib.check(rc)
        for k, name in CTX_NAMES[:6]:
            _eq(again[k], plain[name], "off again " + name)
        _lib.check(L.smx_ctx_set_scanline(ctx, C.byref(_p(**SO))))
        rc, got = _ctx_pair(ctx, ts, L.smx_ctx_stereo_pair, gray, 0, True)
        _lib.check(rc)
        sl, sr = ts["want"]("scanline", None, "gray", **SO)
        _eq(got["agg_l"], sl["agg"], "on again aggl")
        _eq(got["dmap_r"], sr["z"].astype(np.float32), "on again dmapr")
    finally:
        L.smx_destroy(ctx)
    # more than 256 labels: refused at the pair call
    big = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), 8, 4, 257, C.byref(big)))
    try:
        _lib.check(L.smx_ctx_set_scanline(big, C.byref(_p())))
        g = np.zeros((4, 8), np.uint8)
        bufs = {k: np.empty((4, 8), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        assert L.smx_ctx_stereo_pair(big, g.ctypes.data, g.ctypes.data, -256, 0, C.byref(out)) == -1
        assert b"scan-line" in L.smx_last_error()
    finally:
        L.smx_destroy(big)
