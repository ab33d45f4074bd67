"""Region voting and 16-direction interpolation on the GPU (smx_dev_region_vote and everything above it) against
tests/vote_ref.py, bit for bit -- NaN payloads included, since every pixel is either copied or an exact integer.  Every buffer
of a device call lies in a Guarded (tests/guarded.py); the workspace is poisoned and misaligned by 0, 1 or 255 bytes.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cgf_ref
import cross_ref
import fuzz_scenes
import vote_ref as ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
MISALIGN = (0, 1, 255)


def _bits(a, b, name=""):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} pixels differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} != {b.ravel()[bad[:5]]}"


def _p(**kw):
    p = smx.default_vote_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _xp(**kw):
    p = smx.default_cross_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _kw(p):
    return dict(tau_s=p.tau_s, tau_h_pct=p.tau_h_pct, iterations=p.iterations, interpolate_=p.interpolate)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tile():
    tw, th = C.c_int(0), C.c_int(0)
    _lib.check(smx.lib().smx_vote_geometry(C.byref(tw), C.byref(th)))
    return tw.value, th.value


class Call:
    """One smx_dev_region_vote call on guarded buffers"""

    def __init__(self, disp, arms, guide, disp_r, dmin, size_d, d_lr=0, misalign=0, in_place=False, ws_bytes=None):
        h, w = disp.shape
        n = w * h
        self.shape, self.dmin, self.size_d, self.d_lr = (h, w), dmin, size_d, d_lr
        self.ch = 1 if guide.ndim == 2 else guide.shape[2]
        arms = np.ascontiguousarray(arms, np.uint32)
        self.arms = Guarded(n * 4, np.uint8, (n * 4,), plane=n).load(arms.view(np.uint8).reshape(-1))
        self.guide = Guarded(guide.nbytes, np.uint8, guide.shape, plane=n, misalign=3).load(guide)
        self.disp = Guarded(n * 4, np.float32, (h, w), plane=n).load(disp)
        self.right = None if disp_r is None else Guarded(n * 4, np.float32, (h, w), plane=n).load(disp_r)
        self.out = self.disp if in_place else Guarded(n * 4, np.float32, (h, w), plane=n)
        self.in_place = in_place
        self.ws_bytes = int(smx.lib().smx_vote_workspace_bytes(w, h)) if ws_bytes is None else ws_bytes
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0x5A, plane=n)

    def run(self, p):
        h, w = self.shape
        return smx.lib().smx_dev_region_vote(C.byref(p), self.arms.ptr, self.guide.ptr, self.ch, self.disp.ptr,
                                             None if self.right is None else self.right.ptr, self.out.ptr, w, h, self.dmin,
                                             self.size_d, self.d_lr, self.ws.ptr, self.ws_bytes, _stream())

    def check_memory(self):
        self.arms.check_unchanged("d_arms")
        self.guide.check_unchanged("d_guide")
        if self.right is not None:
            self.right.check_unchanged("d_disp_r")
        if self.in_place:
            self.disp.check("d_disp == d_out")
        else:
            self.disp.check_unchanged("d_disp")
            self.out.check("d_out")
        self.ws.check("d_ws")

    def result(self, p):
        _lib.check(self.run(p))
        self.check_memory()
        return self.out.numpy()


def _want(d, arms, g, dr, dmin, D, d_lr, p):
    return ref.region_vote(d, arms, g, dr, dmin, D, d_lr, **_kw(p))


def _check(d, arms, g, dr, dmin, D, p, name, d_lr=0, misalign=0, in_place=False):
    want = _want(d, arms, g, dr, dmin, D, d_lr, p)
    got = Call(d, arms, g, dr, dmin, D, d_lr, misalign, in_place).result(p)
    _bits(got, want, name)
    return want


def _scene_arms(seed, h, w, dmin, D, guide="textured", kind="messy", ch=3, l1=17, **arm_kw):
    g, d, dr = ref.scene(seed, h, w, dmin, D, guide, kind, ch)
    kw = dict(l1=l1, l2=l1 // 2, tau1=20, tau2=6)
    kw.update(arm_kw)
    return g, d, dr, cross_ref.pack_arms(cross_ref.arms(g, **kw))


# ---------------------------------------------------------------------------------------------
# shapes, label ranges, arms
# ---------------------------------------------------------------------------------------------
def _heights():
    _, th = _tile()
    return sorted({1, 2, 70, th - 1, th, th + 1} - {0})


def _widths():
    tw, _ = _tile()
    return sorted({1, 2, 63, 64, 65, 129, tw - 1, tw, tw + 1} - {0})


def test_the_tile_is_what_the_shapes_assume():
    assert _tile() == (64, 4)       # (the lists above follow the hook; this line tells when the kernel's tile changes)


@pytest.mark.parametrize("w", [1, 2, 63, 64, 65, 129])
def test_shapes(w):
    assert set(_widths()) == {1, 2, 63, 64, 65, 129}
    changed = 0
    for k, h in enumerate(_heights()):
        g, d, dr, arms = _scene_arms(100 * w + h, h, w, -3, 8)
        want = _check(d, arms, g, dr, -3, 8, _p(tau_s=3, iterations=3), f"{w} x {h}", misalign=MISALIGN[k % 3])
        changed += int((want.view(np.uint32) != d.view(np.uint32)).sum())
    assert changed > 0 or w == 1


@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 256, 512])
def test_label_ranges(D):
    w, h = 65, 21
    for dmin in (0, -(D // 2) - 3):
        g, d, dr, arms = _scene_arms(D, h, w, dmin, D, kind="plain" if dmin else "messy")
        want = _check(d, arms, g, dr, dmin, D, _p(tau_s=2, tau_h_pct=10 if D > 2 else 40, iterations=2), f"D {D} dmin {dmin}",
                      misalign=MISALIGN[D % 3])
        assert (want != d).any()
        if D >= 63:
            assert len(np.unique(want[ref.voters(want, dmin, D)[0]])) > 10          # bins all over the range are hit


@pytest.mark.parametrize("l1", [1, 17, 63])
@pytest.mark.parametrize("guide", ref.GUIDES)
def test_arms_of_every_kind(guide, l1):
    w, h, D = 70, 40, 12
    for ch in (1, 3):
        g, d, dr, arms = _scene_arms(l1 + ch, h, w, -5, D, guide, "plain", ch, l1=l1)
        _check(d, arms, g, dr, -5, D, _p(tau_s=1 if l1 == 1 else 20, iterations=2), f"{guide} l1 {l1} ch {ch}")


def test_hand_made_arms():
    """any arms that stay inside the image, up to 255 long: longer than smx_dev_cross_arms ever makes them"""
    w, h, D = 300, 9, 6
    rng = np.random.default_rng(9)
    g, d, dr = ref.scene(9, h, w, 0, D, "textured", "plain", 3)
    yy, xx = np.mgrid[0:h, 0:w]
    border = np.stack((xx, w - 1 - xx, yy, h - 1 - yy))
    a = np.minimum(rng.integers(0, 256, (4, h, w)), border)
    assert a.max() > 200
    _check(d, cross_ref.pack_arms(a), g, dr, 0, D, _p(iterations=2), "random arms")
    a = np.minimum(255, border)
    _check(d, cross_ref.pack_arms(a), g, dr, 0, D, _p(iterations=1), "the longest arms")
    _check(d, np.zeros((h, w), np.uint32), g, dr, 0, D, _p(tau_s=0, iterations=3), "no arms")


# ---------------------------------------------------------------------------------------------
# large counts
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    w = h = 130
    g = np.full((h, w), 90, np.uint8)
    arms = cross_ref.pack_arms(cross_ref.arms(g, l1=63, l2=0, tau1=20, tau2=6))
    return g, arms


@pytest.mark.parametrize("D, label", [(8, 5), (512, 511), (512, 0)])
def test_a_count_of_16128(D, label):
    g, arms = _big()
    d = np.full((130, 130), label, F32)
    d[65, 65] = -100
    assert ref.histograms(d, ref.unpack_arms(arms), 0, D)[1][0][65, 65] == 16128
    for tau_s, filled in ((16127, True), (16128, False)):          # the count is exact: S > tau_s
        want = _check(d, arms, g, None, 0, D, _p(tau_s=tau_s, tau_h_pct=99, iterations=1, interpolate=0), f"tau_s {tau_s}")
        assert (want[65, 65] == label) == filled


@pytest.mark.parametrize("D, lo, hi", [(8, 2, 5), (512, 0, 511), (512, 255, 256), (65, 63, 64)])
def test_a_tie_of_8064_each(D, lo, hi):
    g, arms = _big()
    for first, second in ((lo, hi), (hi, lo)):
        d = np.full((130, 130), second, F32)
        d[:65] = first
        d[65, :65] = first
        d[65, 65] = -100
        _, H = ref.histograms(d, ref.unpack_arms(arms), 0, D)
        assert H[:, 65, 65].tolist() == [8064, 8064]
        want = _check(d, arms, g, None, 0, D, _p(tau_s=16127, tau_h_pct=49, iterations=1, interpolate=0), f"{first} | {second}")
        assert want[65, 65] == hi
        want = _check(d, arms, g, None, 0, D, _p(tau_s=16127, tau_h_pct=50, iterations=1, interpolate=0), "50 % is no majority")
        assert want[65, 65] == -100


# ---------------------------------------------------------------------------------------------
# extremes and map kinds
# ---------------------------------------------------------------------------------------------
def test_extremes():
    w, h, D = 70, 23, 8
    g, d, dr, arms = _scene_arms(4, h, w, 0, D, kind="plain")
    every = np.full((h, w), -100, F32)
    _bits(_check(every, arms, g, dr, 0, D, _p(tau_s=0, tau_h_pct=0), "every pixel an outlier"), every, "nothing changes")
    none = np.where(ref.valid(d, 0), d, F32(3)).astype(F32)
    _bits(_check(none, arms, g, dr, 0, D, _p(tau_s=0), "no outlier"), none, "a copy")
    border = none.copy()
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = -100
    want = _check(border, arms, g, dr, 0, D, _p(tau_s=2), "outliers on the border")
    assert ref.valid(want, 0).all()
    nobody = np.full((h, w), D, F32)                          # valid everywhere, no voter anywhere
    nobody[5:9, 5:30] = np.nan
    _bits(_check(nobody, arms, g, dr, 0, D, _p(tau_s=0, tau_h_pct=0), "no voter"), nobody, "nothing changes")


MAP_KINDS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "-0": -0.0, "fraction": 2.75, "negative fraction": -0.5,
             "beyond int": 3e9, "below int": -3e9, "behind the range": 8.0, "2^31": 2147483648.0, "marker": -100.0}


@pytest.mark.parametrize("kind", sorted(MAP_KINDS))
def test_map_kinds(kind):
    """a third of the pixels hold the value, as outliers or as voters or as neither, whatever it is"""
    w, h, D = 66, 13, 8
    for dmin in (0, -4):
        g, d, dr, arms = _scene_arms(len(kind), h, w, dmin, D, kind="plain")
        m = np.random.default_rng(3).random((h, w)) < 0.33
        d = np.where(m, F32(MAP_KINDS[kind]), d).astype(F32)
        dr = np.where(m[:, ::-1], F32(MAP_KINDS[kind]), dr).astype(F32)
        _check(d, arms, g, dr, dmin, D, _p(tau_s=3, iterations=2), f"{kind} dmin {dmin}")


# ---------------------------------------------------------------------------------------------
# parameters and forms of the call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 1, 2, 5, 8])
def test_iterations_interpolation_right_map_and_channels(iterations):
    w, h, D = 67, 22, 8
    seen = set()
    for k, (interpolate, right, ch) in enumerate([(i, r, c) for i in (0, 1) for r in (True, False) for c in (1, 3, 4)]):
        g, d, dr, arms = _scene_arms(40 + ch, h, w, -2, D, ch=ch, l1=3)
        p = _p(tau_s=4, iterations=iterations, interpolate=interpolate)
        want = _check(d, arms, g, dr if right else None, -2, D, p, f"iterations {iterations} interpolate {interpolate} right "
                      f"{right} ch {ch}", d_lr=k % 2, misalign=MISALIGN[k % 3])
        seen.add(want.tobytes())
    assert len(seen) >= (3 if iterations < 8 else 2)          # the forms differ


def test_the_rounds_move_the_front_one_pixel_each():
    """tests/test_vote_cpu.py's Jacobi row on the GPU: in place too, a round reads M_k only"""
    d = np.full((1, 30), -100, F32)
    d[0, :6] = 3
    g = np.full((1, 30), 7, np.uint8)
    arms = cross_ref.pack_arms(cross_ref.arms(g, l1=3, l2=0, tau1=20, tau2=6))
    for it in (1, 2, 8):
        for in_place in (False, True):
            want = _check(d, arms, g, None, 0, 8, _p(tau_s=2, iterations=it, interpolate=0), f"{it} rounds", in_place=in_place)
            assert (want[0] == 3).sum() == 6 + it


def test_in_place_equals_out_of_place():
    w, h, D = 129, 33, 16
    g, d, dr, arms = _scene_arms(77, h, w, -15, D)
    for p in (_p(), _p(iterations=0), _p(interpolate=0), _p(iterations=0, interpolate=0), _p(iterations=1)):
        want = _want(d, arms, g, dr, -15, D, 0, p)
        for in_place in (False, True):
            _bits(Call(d, arms, g, dr, -15, D, in_place=in_place, misalign=255).result(p), want, f"in place {in_place}")


def test_a_workspace_one_byte_short():
    w, h, D = 40, 9, 4
    g, d, dr, arms = _scene_arms(1, h, w, 0, D)
    L = smx.lib()
    need = int(L.smx_vote_workspace_bytes(w, h))
    assert need == 255 + 8 * w * h
    call = Call(d, arms, g, dr, 0, D, ws_bytes=need - 1)
    assert call.run(_p()) == -3 and b"workspace" in L.smx_last_error()
    call.check_memory()
    call.out.check_untouched("d_out")
    call.ws.check_untouched("d_ws")
    call = Call(d, arms, g, dr, 0, D, ws_bytes=need, misalign=255)             # ... and exactly that many bytes are enough
    _bits(call.result(_p()), _want(d, arms, g, dr, 0, D, 0, _p()), "smallest workspace")


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    import torch
    w, h, D = 129, 40, 16
    g, d, dr, arms = _scene_arms(5, h, w, -15, D)
    p = _p()
    want = _want(d, arms, g, dr, -15, D, 0, p)
    call = Call(d, arms, g, dr, -15, D, misalign=1)
    _bits(call.result(p), want, "first run")
    call.out.view.zero_()
    call.ws.bytes.fill_(0x11)
    _bits(call.result(p), want, "second run")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.check(call.run(p))                 # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(call.run(p))
    for fill in (0x77, 0x00):
        call.out.view.zero_()
        call.ws.bytes.fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        _bits(call.out.numpy(), want, "graph replay")
    call.check_memory()


# ---------------------------------------------------------------------------------------------
# the host entry and the numpy front end
# ---------------------------------------------------------------------------------------------
def test_host_pointer_entry_and_stages():
    w, h, D = 45, 31, 6
    L = smx.lib()
    for ch in (1, 3, 4):
        g, d, dr = ref.scene(ch, h, w, -5, D, "textured", "messy", ch)
        xp = _xp(l1=9, l2=4, iterations=3)
        p = _p(tau_s=5)
        want = ref.region_vote_guide(d, g, dr, -5, D, 1, cross=dict(l1=9, l2=4, tau1=20, tau2=6), **_kw(p))
        out = np.empty((h, w), F32)
        _lib.check(L.smx_region_vote(C.byref(p), C.byref(xp), g.ctypes.data, ch, d.ctypes.data, dr.ctypes.data, out.ctypes.data,
                                     w, h, -5, D, 1))
        _bits(out, want, f"host entry ch {ch}")
        _bits(smx.region_vote(d, g, -5, D, disparity_right=dr, d_lr=1, params=p, arms=xp), want, f"stages ch {ch}")
    # the defaults, no right map, a gray guide as (h, w); in place through the host entry
    g, d, dr = ref.scene(8, h, w, 0, D, "textured", "plain", 1)
    want = ref.region_vote_guide(d, g, None, 0, D, 0)
    _bits(smx.region_vote(d, g, 0, D), want, "defaults")
    _bits(smx.region_vote(d, g[:, :, None], 0, D), want, "(h, w, 1)")
    buf = d.copy()
    _lib.check(L.smx_region_vote(C.byref(_p()), None, g.ctypes.data, 1, buf.ctypes.data, None, buf.ctypes.data, w, h, 0, D, 0))
    _bits(buf, want, "in place")
    assert (want != d).any()


def test_the_block_beside_the_step_on_the_gpu():
    from test_vote_cpu import step_case
    g, d, truth, block = step_case()
    filled = smx.fill_occlusion(d, 0)
    assert (filled[block] != truth[block]).all()
    voted = smx.region_vote(d, g, 0, 8, arms=_xp(l1=17, l2=8))
    assert np.array_equal(smx.fill_occlusion(voted, 0), truth.astype(F32))


# ---------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------
from test_gpu_cross import CTX_NAMES, PD, PDMINL, PH, PW, _ctx_create, _ctx_pair, _t          # noqa: E402

VOTE = dict(tau_s=10, tau_h_pct=40, iterations=3, interpolate=1)
ARMS = dict(l1=17, l2=8, tau1=20, tau2=6)
AGGS = {"guided": {}, "guided rgb": dict(guidance="rgb"), "sgm": dict(aggregation="sgm"), "cross": dict(aggregation="cross")}


@pytest.fixture(scope="module")
def pair(orc):
    rgb_l, rgb_r = cgf_ref.colour_pair(PW, PH, PD, 4711)
    return dict(rgb=(rgb_l, rgb_r), Il=orc.gray(rgb_l), Ir=orc.gray(rgb_r))


def _pipe(pair, agg, **kw):
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, want_agg=True, **AGGS[agg], **kw)
    rgb = dict(rgb_l=_t(pair["rgb"][0]), rgb_r=_t(pair["rgb"][1])) if agg == "guided rgb" else {}
    return pipe, (_t(pair["Il"]), _t(pair["Ir"])), rgb


def _chain_of(orc, pair, agg, got, d_lr, **stages):
    """vote_ref.chain behind the winners the pipeline found (the aggregations have their own tests)"""
    st = cgf_ref.states(got["aggl"])
    e = dict(dmapl=got["dmapl"], dmapr=got["dmapr"], grayl=pair["Il"])
    guide = pair["rgb"][0] if agg == "guided rgb" else pair["Il"]
    vote = {("interpolate_" if k == "interpolate" else k): v for k, v in VOTE.items()}
    return ref.chain(orc, e, PDMINL, PD, guide, vote, ARMS, d_lr, z=st["z"], best=st["best"], sec=st["uq"][0], nbr=st["nbr"][:2],
                     **stages)


@pytest.mark.parametrize("agg", sorted(AGGS))
@pytest.mark.parametrize("cost", [None, "census", "adcensus"])
def test_pipeline(orc, pair, cost, agg):
    pipe, imgs, rgb = _pipe(pair, agg, cost=cost, vote=_p(**VOTE), vote_arms=_xp(**ARMS))
    pipe.run(*imgs, **rgb)
    got = pipe.results()
    want = _chain_of(orc, pair, agg, got, int(pipe.params.d_lr))
    for k in ("occlusion", "voted", "filled"):
        _bits(got[k], want[k], f"cost {cost} aggregation {agg} {k}")
    assert (want["voted"] != want["occlusion"]).any()
    assert pipe.vote_ws is not None and pipe.vote_ws_bytes == 255 + 8 * PW * PH


def test_composition_with_uniqueness_speckle_subpixel_and_weighted_median(orc, pair):
    spk = _lib.SpeckleParams()
    spk.max_size, spk.max_diff = 30, 1.0
    kw = dict(cost="adcensus", vote=_p(**VOTE), vote_arms=_xp(**ARMS), speckle=spk, uniqueness=fuzz_scenes.ratio_of(5),
              subpixel="parabola", wmf="occluded")
    want = None           # (5 %: with this pair's AD-Census costs 15 % leaves no valid pixel to vote)
    for sif, per_call in ((None, False), (5, False), (3, True)):          # chunked against unchunked; the per-stage finish
        pipe, imgs, rgb = _pipe(pair, "cross", slices_in_flight=sif, **kw)
        pipe.aggregate(*imgs, **rgb)
        if per_call:
            pipe.finish_per_call()
            pipe.subpixel_maps()
            pipe.refine()
        else:
            pipe.finish()
        got = pipe.results()
        if want is None:
            want = _chain_of(orc, pair, "cross", got, int(pipe.params.d_lr), uniqueness=5, speckle=(30, 1.0), subpixel="parabola",
                             wmf="occluded")
        for k, name in (("occlusion",) * 2, ("unique",) * 2, ("despeckled",) * 2, ("voted",) * 2, ("filled",) * 2,
                        ("subpix_filled", "sub_filled"), ("refined",) * 2):
            _bits(got[k], want[name], f"slices in flight {sif} per call {per_call}: {k}")
    assert (want["voted"] != want["despeckled"]).any() and (want["unique"] != want["occlusion"]).any()
    # a voted pixel gets no sub-pixel offset, and stays a pixel for the weighted median
    filled_only = ~ref.valid(want["despeckled"], PDMINL)
    _bits(want["sub_filled"][filled_only], want["filled"][filled_only], "no offset where the map was not valid")


def test_vote_off_allocates_and_launches_nothing(orc, pair):
    pipe, imgs, rgb = _pipe(pair, "guided")
    assert pipe.vote is None and pipe.voted is None and pipe.vote_ws is None and pipe.vote_arms_plane is None
    pipe.run(*imgs)
    got = pipe.results()
    assert "voted" not in got
    want = orc.stereo_pair(pair["Il"], pair["Ir"], PD, dminl=PDMINL, dminr=0)
    for k in ("dmapl", "dmapr", "occlusion", "filled"):
        _bits(got[k], want[k], k)
    true, _, _ = _pipe(pair, "guided", vote=True)
    assert (true.vote.tau_s, true.vote.iterations, true.vote_arms.l1) == (20, 5, 34)


def test_pipeline_on_tsukuba(orc, tsukuba_gray, tsukuba_oracle):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = tsukuba_gray
    h, w = Il.shape
    pipe = PairPipeline(w, h, 16, dminl=-15, vote=True)
    pipe.run(_t(Il), _t(Ir))
    got = pipe.results()
    _bits(got["occlusion"], tsukuba_oracle["occlusion"], "occlusion")
    voted = ref.region_vote_guide(tsukuba_oracle["occlusion"], Il, tsukuba_oracle["dmapr"], -15, 16, int(pipe.params.d_lr))
    _bits(got["voted"], voted, "voted")
    _bits(got["filled"], orc.fill_occlusion(voted, -15), "filled")
    out = ~ref.valid(tsukuba_oracle["occlusion"], -15)
    assert out.sum() > 1000 and ref.valid(voted, -15)[out].mean() > 0.9


def test_the_sharded_driver_refuses():
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError, match="region voting"):
        ShardedPair(PW, PH, PD, vote=True)


# ---------------------------------------------------------------------------------------------
# the context
# ---------------------------------------------------------------------------------------------
def _voted_of(ctx):
    v = np.empty((PH, PW), F32)
    _lib.check(smx.lib().smx_ctx_vote_map(ctx, v.ctypes.data))
    return v


def test_context(orc, pair):
    L = smx.lib()
    ctx = _ctx_create()
    gray, rgb = (pair["Il"], pair["Ir"]), pair["rgb"]
    d_lr = int(smx.default_params().d_lr)
    vote = {("interpolate_" if k == "interpolate" else k): v for k, v in VOTE.items()}
    try:
        rc, off = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        plain = orc.stereo_pair(*gray, PD, dminl=PDMINL, dminr=0)
        for k, name in CTX_NAMES:
            _bits(off[k], plain[name], "off " + name)
        assert L.smx_ctx_vote_map(ctx, None) == -1 and b"without region voting" in L.smx_last_error()
        for bad in (dict(tau_s=-1), dict(tau_h_pct=100), dict(iterations=9), dict(interpolate=2)):
            assert L.smx_ctx_set_vote(ctx, C.byref(_p(**bad)), None) == -1
        assert L.smx_ctx_set_vote(ctx, C.byref(_p()), C.byref(_xp(l1=64))) == -1
        rc, still = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)          # a refused setter leaves it off
        _lib.check(rc)
        _bits(still["filled"], plain["filled"], "still off")
        # on: the gray entry with the gray guide, the colour entry with the colour guide
        _lib.check(L.smx_ctx_set_vote(ctx, C.byref(_p(**VOTE)), C.byref(_xp(**ARMS, iterations=77))))
        assert L.smx_ctx_stereo_pair_async(ctx, gray[0].ctypes.data, gray[1].ctypes.data, PDMINL, 0) == -1
        assert b"smx_ctx_set_vote" in L.smx_last_error()
        for entry, imgs, ch, guide in ((L.smx_ctx_stereo_pair, gray, 0, gray[0]), (L.smx_ctx_stereo_pair_rgb, rgb, 3, rgb[0])):
            rc, on = _ctx_pair(ctx, entry, imgs, ch, False)
            _lib.check(rc)
            for k, name in CTX_NAMES[:5]:
                _bits(on[k], plain[name], "on " + name)                     # (occlusion stays the LR-check map)
            voted = ref.region_vote_guide(plain["occlusion"], guide, plain["dmapr"], PDMINL, PD, d_lr, cross=ARMS, **vote)
            _bits(_voted_of(ctx), voted, f"voted, {ch} channels")
            _bits(on["filled"], orc.fill_occlusion(voted, PDMINL), f"filled, {ch} channels")
            assert (voted != plain["occlusion"]).any()
        # behind speckle removal, with cross-based aggregation and the AD-Census cost
        spk = _lib.SpeckleParams()
        spk.max_size, spk.max_diff = 30, 1.0
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(spk)))
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(smx.default_cross_params())))
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())))
        rc, on = _ctx_pair(ctx, L.smx_ctx_stereo_pair_rgb, rgb, 3, False)
        _lib.check(rc)
        spk_map = np.empty((PH, PW), F32)
        _lib.check(L.smx_ctx_speckle_map(ctx, spk_map.ctypes.data))
        voted = ref.region_vote_guide(spk_map, rgb[0], on["dmap_r"], PDMINL, PD, d_lr, cross=ARMS, **vote)
        _bits(_voted_of(ctx), voted, "voted behind speckle removal")
        _bits(on["filled"], orc.fill_occlusion(voted, PDMINL), "filled behind speckle removal")
        _lib.check(L.smx_ctx_set_speckle(ctx, None))
        _lib.check(L.smx_ctx_set_cross(ctx, None))
        _lib.check(L.smx_ctx_set_adcensus(ctx, None))
        # off, and on again with the defaults
        _lib.check(L.smx_ctx_set_vote(ctx, None, None))
        rc, again = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        for k, name in CTX_NAMES:
            _bits(again[k], plain[name], "off again " + name)
        assert L.smx_ctx_vote_map(ctx, None) == -1
        _lib.check(L.smx_ctx_set_vote(ctx, C.byref(_p()), None))
        rc, on = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        _bits(_voted_of(ctx), ref.region_vote_guide(plain["occlusion"], gray[0], plain["dmapr"], PDMINL, PD, d_lr), "the defaults")
    finally:
        L.smx_destroy(ctx)


def test_a_context_of_more_than_512_labels_refuses():
    L = smx.lib()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), 40, 8, 513, C.byref(ctx)))
    try:
        assert L.smx_ctx_set_vote(ctx, C.byref(_p()), None) == -1 and b"size_d" in L.smx_last_error()
    finally:
        L.smx_destroy(ctx)
