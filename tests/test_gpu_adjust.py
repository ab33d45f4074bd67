"""The depth-discontinuity adjustment on the GPU (smx_dev_discontinuity_adjust and everything above it) against
tests/adjust_ref.py, bit for bit -- every pixel is either copied or takes a neighbour's bits, and the sub-pixel map is one f32
formula.  Every buffer of a device call lies in a Guarded (tests/guarded.py); the workspace is poisoned with 0xFF and misaligned
by 0, 1 or 255 bytes.
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import adjust_ref as ref
import cgf_ref
import fuzz_scenes
import subpix_ref
import vote_ref
import wmf_ref
from guarded import Guarded
from test_adjust_cpu import BLOCK, DMIN, SIZE_D, STEP_COUNTS, random_case, step_case

pytestmark = pytest.mark.gpu

F32 = np.float32
MISALIGN = (0, 1, 255)
MODES = {None: 0, "parabola": subpix_ref.PARABOLA, "equiangular": subpix_ref.EQUIANGULAR}


def _bits(a, b, name=""):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} pixels differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} != {b.ravel()[bad[:5]]}"


def _p(**kw):
    p = smx.default_adjust_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _kw(p):
    return dict(tau_e=p.tau_e, vertical=p.vertical, iterations=p.iterations)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tile():
    tw, th = C.c_int(0), C.c_int(0)
    _lib.check(smx.lib().smx_adjust_geometry(C.byref(tw), C.byref(th)))
    return tw.value, th.value


class Call:
    """One smx_dev_discontinuity_adjust call on guarded buffers"""

    def __init__(self, disp, vol, dmin, mode=None, sub=None, misalign=0, in_place=False, ws_bytes=None):
        h, w = disp.shape
        n = w * h
        self.shape, self.dmin, self.size_d, self.mode = (h, w), dmin, vol.shape[0], MODES[mode]
        self.disp = Guarded(n * 4, np.float32, (h, w), plane=n).load(disp)
        self.vol = Guarded(vol.nbytes, np.float32, vol.shape, plane=n).load(vol)
        self.out = self.disp if in_place else Guarded(n * 4, np.float32, (h, w), plane=n)
        self.sub = None if sub is None else Guarded(n * 4, np.float32, (h, w), plane=n).load(sub)
        self.in_place = in_place
        self.ws_bytes = int(smx.lib().smx_adjust_workspace_bytes(w, h)) if ws_bytes is None else ws_bytes
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0xFF, plane=n)

    def run(self, p):
        h, w = self.shape
        return smx.lib().smx_dev_discontinuity_adjust(C.byref(p), self.disp.ptr, self.vol.ptr, self.out.ptr, w, h, self.dmin,
                                                      self.size_d, self.mode, None if self.sub is None else self.sub.ptr,
                                                      self.ws.ptr, self.ws_bytes, _stream())

    def check_memory(self):
        self.vol.check_unchanged("d_agg")
        if self.in_place:
            self.disp.check("d_disp == d_out")
        else:
            self.disp.check_unchanged("d_disp")
            self.out.check("d_out")
        if self.sub is not None:
            self.sub.check("d_sub")
        self.ws.check("d_ws")

    def result(self, p):
        _lib.check(self.run(p))
        self.check_memory()
        return self.out.numpy() if self.sub is None else (self.out.numpy(), self.sub.numpy())


def _check(d, vol, dmin, p, name, mode=None, sub=None, misalign=0, in_place=False):
    """-> the reference's map (and its sub-pixel map), which the kernel's equal"""
    if sub is None:
        want = ref.adjust(d, vol, dmin, **_kw(p))
        _bits(Call(d, vol, dmin, misalign=misalign, in_place=in_place).result(p), want, name)
        return want
    want, wsub = ref.adjust(d, vol, dmin, mode=MODES[mode], sub=sub, **_kw(p))
    got, gsub = Call(d, vol, dmin, mode, sub, misalign, in_place).result(p)
    _bits(got, want, name)
    _bits(gsub, wsub, name + " sub")
    return want, wsub


def _changed(want, d):
    return int((want.view(np.uint32) != d.view(np.uint32)).sum())


# ---------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------
def test_the_footprint_is_what_the_shapes_assume():
    assert _tile() == (64, 4)       # (the seam shapes below follow the hook; this line tells when the kernel's footprint changes)


@pytest.mark.parametrize("w", [1, 2, 3, 63, 64, 65, 129])
def test_shapes(w):
    changed = 0
    for k, h in enumerate((1, 2, 5, 70)):
        rng = np.random.default_rng(100 * w + h)
        d, vol = random_case(rng, h, w, -3, 8)
        want = _check(d, vol, -3, _p(tau_e=1 + k % 2, iterations=1 + k % 3), f"{w} x {h}", misalign=MISALIGN[k % 3])
        changed += _changed(want, d)
    assert changed > 0


def seam_case(rng, h, w, cols, rows, dmin, size_d):
    """a label per workgroup footprint, so that every depth step lies on a seam between two of them, in both axes"""
    yy, xx = np.mgrid[0:h, 0:w]
    d = (dmin + (3 * (xx // cols) + 5 * (yy // rows)) % size_d).astype(F32)
    vol = rng.integers(0, 4, (size_d, h, w)).astype(F32)
    return d, vol


def test_depth_steps_on_the_seams_between_workgroups():
    cols, rows = _tile()
    rng = np.random.default_rng(11)
    for k, (w, h) in enumerate([(w, h) for w in (cols - 1, cols, cols + 1, 2 * cols + 1) for h in (rows - 1, rows, rows + 1, 3 * rows)]):
        d, vol = seam_case(rng, h, w, cols, rows, -2, 8)
        sub = rng.normal(size=(h, w)).astype(F32)
        for vertical in (0, 1):
            stats = {}
            ref.adjust(d, vol, -2, 2, vertical, 1, stats=stats)
            want, _ = _check(d, vol, -2, _p(tau_e=2, vertical=vertical, iterations=2), f"{w} x {h} vertical {vertical}", "parabola", sub,
                             misalign=MISALIGN[k % 3], in_place=bool(k % 2))
            if w > cols:
                assert stats["changed_h"] > 0 and stats["candidate_h"] > stats["changed_h"]
            if h > rows and vertical:
                assert stats["changed_v"] > 0
            assert stats.get("candidate_v", 0) == 0 or vertical


# ---------------------------------------------------------------------------------------------
# label ranges and parameters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 64, 65, 256, 512])
def test_label_ranges(D):
    w, h = 65, 9
    for k, dmin in enumerate((-(D // 2) - 3, 0, 7)):
        rng = np.random.default_rng(D + k)
        d, vol = random_case(rng, h, w, dmin, D, block=(2, 4))
        sub = rng.normal(size=(h, w)).astype(F32)
        for tau_e in sorted({1, 2, D}):
            want, wsub = _check(d, vol, dmin, _p(tau_e=tau_e, iterations=2), f"D {D} dmin {dmin} tau_e {tau_e}", "equiangular", sub,
                                misalign=MISALIGN[(D + k) % 3])
            if tau_e >= D:
                _bits(want, d, "no step reaches tau_e = size_d: a copy")
                _bits(wsub, sub, "and the sub-pixel map is untouched")
            elif tau_e == 1:
                assert _changed(want, d) > 0
                lab, z = ref.labelled(want, dmin, D)
                moved = lab & (want.view(np.uint32) != d.view(np.uint32))
                if D >= 64:
                    assert z[moved].min() < D // 4 and z[moved].max() >= D - D // 4     # changed pixels all over the range


@pytest.mark.parametrize("iterations", [1, 2, 8])
@pytest.mark.parametrize("vertical", [0, 1])
def test_iterations_vertical_in_place_and_the_sub_pixel_modes(iterations, vertical):
    w, h, D = 67, 22, 9
    seen = set()
    for k, (mode, in_place) in enumerate([(m, i) for m in (None, "parabola", "equiangular") for i in (False, True)]):
        rng = np.random.default_rng(40)
        d, vol = random_case(rng, h, w, -4, D)
        sub = None if mode is None else rng.normal(size=(h, w)).astype(F32)
        p = _p(tau_e=2, vertical=vertical, iterations=iterations)
        want = _check(d, vol, -4, p, f"iterations {iterations} vertical {vertical} {mode} in place {in_place}", mode, sub,
                      misalign=MISALIGN[k % 3], in_place=in_place)
        if mode is not None:
            want, wsub = want
            assert (wsub.view(np.uint32) != sub.view(np.uint32)).sum() > 0
            seen.add(wsub.tobytes())
        assert _changed(want, d) > 0
    assert len(seen) == 2                                   # the two fits differ


def test_the_rounds_move_an_edge_one_pixel_each():
    """tests/test_adjust_cpu.py's row on the GPU: in place too, a round reads the snapshot only"""
    d = np.array([[1] * 3 + [5] * 27], F32)
    vol = np.full((8, 1, 30), 9, F32)
    vol[1] = 2
    for it in (1, 2, 8):
        for in_place in (False, True):
            want = _check(d, vol, 0, _p(iterations=it), f"{it} rounds", in_place=in_place)
            assert (want[0] == 1).sum() == 3 + it
    # and a pixel's own cost never rises from round to round
    rng = np.random.default_rng(8)
    d, vol = random_case(rng, 30, 70, -4, 9, specials=False)
    cost = ref.own_cost(d, vol, -4)
    for it in range(1, 9):
        got = Call(d, vol, -4).result(_p(tau_e=1, iterations=it))
        nxt = ref.own_cost(got, vol, -4)
        assert (nxt[~np.isnan(nxt)] <= cost[~np.isnan(cost)]).all(), it
        cost = nxt


# ---------------------------------------------------------------------------------------------
# extremes
# ---------------------------------------------------------------------------------------------
COSTS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "-0": -0.0, "denormal": float(np.uint32(1).view(F32)),
         "negative denormal": -float(np.uint32(0x7FFFFF).view(F32))}


@pytest.mark.parametrize("kind", sorted(COSTS))
def test_special_costs(kind):
    """a third of the volume holds the value, as own costs and as candidates' costs"""
    w, h, D = 66, 13, 8
    rng = np.random.default_rng(len(kind))
    d, vol = random_case(rng, h, w, -4, D, specials=False)
    vol[rng.random(vol.shape) < 0.33] = COSTS[kind]
    sub = rng.normal(size=(h, w)).astype(F32)
    for mode in ("parabola", "equiangular"):
        _check(d, vol, -4, _p(tau_e=1, iterations=2), f"{kind} {mode}", mode, sub)


def test_the_copies():
    w, h, D = 70, 23, 8
    rng = np.random.default_rng(4)
    _, vol = random_case(rng, h, w, 0, D)
    sub = rng.normal(size=(h, w)).astype(F32)
    kinds = np.array([-100, 2.5, 8, -1, np.nan, np.inf, -np.inf, 3e9], F32)
    unlabelled = kinds[rng.integers(0, len(kinds), (h, w))]
    unlabelled.view(np.uint32)[0, :4] = (0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF812345)      # NaN payloads are bits too
    for name, d in (("all unlabelled", unlabelled), ("all equal", np.full((h, w), 3, F32)), ("all -0", np.full((h, w), -0.0, F32))):
        for in_place in (False, True):
            want, wsub = _check(d, vol, 0, _p(tau_e=1, iterations=3), name, "parabola", sub, in_place=in_place)
            _bits(want, d, name + ": a copy")
            _bits(wsub, sub, name + ": the sub-pixel map is untouched")


def test_in_place_equals_out_of_place():
    w, h, D = 129, 33, 16
    rng = np.random.default_rng(77)
    d, vol = random_case(rng, h, w, -15, D)
    for p in (_p(), _p(iterations=2), _p(iterations=8, tau_e=1), _p(vertical=0)):
        want = ref.adjust(d, vol, -15, **_kw(p))
        for in_place in (False, True):
            _bits(Call(d, vol, -15, in_place=in_place, misalign=255).result(p), want, f"in place {in_place}")
        assert _changed(want, d) > 0


def test_a_workspace_one_byte_short():
    w, h, D = 40, 9, 4
    rng = np.random.default_rng(1)
    d, vol = random_case(rng, h, w, 0, D)
    L = smx.lib()
    need = int(L.smx_adjust_workspace_bytes(w, h))
    assert need == 255 + 8 * w * h
    for in_place in (False, True):
        call = Call(d, vol, 0, ws_bytes=need - 1, in_place=in_place)
        assert call.run(_p()) == -3 and b"workspace" in L.smx_last_error()
        call.vol.check_unchanged("d_agg")
        call.disp.check_unchanged("d_disp")
        if not in_place:
            call.out.check_untouched("d_out")
        call.ws.check_untouched("d_ws")
    for in_place in (False, True):                                      # ... and exactly that many bytes are enough
        call = Call(d, vol, 0, ws_bytes=need, misalign=255, in_place=in_place)
        _bits(call.result(_p(iterations=3)), ref.adjust(d, vol, 0, iterations=3), "smallest workspace")


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    import torch
    w, h, D = 129, 40, 16
    rng = np.random.default_rng(5)
    d, vol = random_case(rng, h, w, -15, D)
    sub = rng.normal(size=(h, w)).astype(F32)
    p = _p(iterations=3)
    want, wsub = ref.adjust(d, vol, -15, mode=subpix_ref.PARABOLA, sub=sub, **_kw(p))
    call = Call(d, vol, -15, "parabola", sub, misalign=1)
    got, gsub = call.result(p)
    _bits(got, want, "first run")
    _bits(gsub, wsub, "first run sub")

    def reset(fill):
        call.out.view.zero_()
        call.sub.load(sub)
        call.ws.bytes.fill_(fill)

    reset(0x11)
    got, gsub = call.result(p)
    _bits(got, want, "second run")
    _bits(gsub, wsub, "second run sub")
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
        reset(fill)
        graph.replay()
        torch.cuda.synchronize()
        _bits(call.out.numpy(), want, "graph replay")
        _bits(call.sub.numpy(), wsub, "graph replay sub")
    call.check_memory()


def test_a_graph_capture_in_place():
    """d_out == d_disp puts a device-to-device copy in front of the launches: it is captured with them, and a second replay
    adjusts the first one's result"""
    import torch
    w, h, D = 129, 40, 16
    rng = np.random.default_rng(6)
    d, vol = random_case(rng, h, w, -15, D)
    p = _p(tau_e=1, iterations=2)
    once = ref.adjust(d, vol, -15, **_kw(p))
    twice = ref.adjust(once, vol, -15, **_kw(p))
    assert _changed(once, d) > 0 and _changed(twice, once) > 0
    call = Call(d, vol, -15, misalign=255, in_place=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _lib.check(call.run(p))                 # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _bits(call.out.numpy(), once, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(call.run(p))
    call.disp.bytes.copy_(call.disp.content)    # the captured call has not run: start over from the input
    call.ws.bytes.fill_(0x33)
    for want, name in ((once, "first replay"), (twice, "second replay")):
        graph.replay()
        torch.cuda.synchronize()
        _bits(call.out.numpy(), want, name)
    call.vol.check_unchanged("d_agg")
    call.disp.check("d_disp == d_out")
    call.ws.check("d_ws")


# ---------------------------------------------------------------------------------------------
# the host entry and the numpy front end
# ---------------------------------------------------------------------------------------------
def test_host_pointer_entry_and_stages():
    w, h, D = 45, 31, 6
    L = smx.lib()
    rng = np.random.default_rng(2)
    d, vol = random_case(rng, h, w, -5, D)
    sub = rng.normal(size=(h, w)).astype(F32)
    p = _p(tau_e=1, iterations=2)
    want, wsub = ref.adjust(d, vol, -5, mode=subpix_ref.EQUIANGULAR, sub=sub, **_kw(p))
    out, s = np.empty((h, w), F32), sub.copy()
    _lib.check(L.smx_discontinuity_adjust(C.byref(p), d.ctypes.data, vol.ctypes.data, out.ctypes.data, w, h, -5, D,
                                          subpix_ref.EQUIANGULAR, s.ctypes.data))
    _bits(out, want, "host entry")
    _bits(s, wsub, "host entry sub")
    got, gsub = smx.discontinuity_adjust(d, vol, -5, params=p, subpixel="equiangular", sub=sub)
    _bits(got, want, "stages")
    _bits(gsub, wsub, "stages sub")
    _bits(smx.discontinuity_adjust(d, vol, -5, params=p), want, "stages without a sub-pixel map")
    _bits(smx.discontinuity_adjust(d, vol, -5), ref.adjust(d, vol, -5), "the defaults")
    buf = d.copy()                                                      # in place through the host entry
    _lib.check(L.smx_discontinuity_adjust(C.byref(p), buf.ctypes.data, vol.ctypes.data, buf.ctypes.data, w, h, -5, D, 0, None))
    _bits(buf, want, "in place")
    assert _changed(want, d) > 0


def test_the_block_beside_the_step_on_the_gpu(orc):
    filled, vol, truth, rejected = step_case(orc)
    _bits(smx.fill_occlusion(rejected, DMIN), filled, "the fill")
    wrong = [int((filled[BLOCK] != truth[BLOCK]).sum())]
    for it in (1, 8):
        out = smx.discontinuity_adjust(filled, vol, DMIN, params=_p(iterations=it))
        wrong.append(int((out[BLOCK] != truth[BLOCK]).sum()))
    assert tuple(wrong) == STEP_COUNTS
    assert np.array_equal(out, truth) and vol.shape[0] == SIZE_D


# ---------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------
from test_gpu_cross import CTX_NAMES, PD, PDMINL, PH, PW, _ctx_create, _ctx_pair, _t          # noqa: E402

ADJ = dict(tau_e=1, vertical=1, iterations=2)
AGGS = {"guided": {}, "sgm": dict(aggregation="sgm"), "cross-scanline": dict(aggregation="cross-scanline")}


def _chain(orc, Il, got, dminl, D, adjust, subpixel=None, wmf=None, vote=None, **stages):
    """The chained numpy references behind the winners of the volume the pipeline kept (the aggregations have their own
    tests): LR check -> uniqueness -> speckle -> vote -> fill -> sub-pixel fit, then the adjustment, then the weighted median."""
    import main_harness
    st = cgf_ref.states(got["aggl"])
    e = dict(dmapl=got["dmapl"], dmapr=got["dmapr"], grayl=Il)
    kw = dict(z=st["z"], best=st["best"], sec=st["uq"][0], nbr=st["nbr"][:2], subpixel=subpixel, **stages)
    if vote is not None:
        vote_ref.chain(orc, e, dminl, D, Il, *vote, **kw)
    else:
        main_harness.finish_chain(orc, e, dminl, D, **kw)
    e["before"] = e["filled"]
    if subpixel:
        e["filled"], e["sub_filled"] = ref.adjust(e["before"], got["aggl"], dminl, mode=subpix_ref.MODES[subpixel], sub=e["sub_filled"],
                                                  **adjust)
    else:
        e["filled"] = ref.adjust(e["before"], got["aggl"], dminl, **adjust)
    if wmf:
        kept = e["despeckled"] if stages.get("speckle") else e["unique"] if stages.get("uniqueness") else e["occlusion"]
        e["refined"] = wmf_ref.weighted_median(Il, e["filled"], dminl, D, kept if wmf == "occluded" else None)
    return e


@pytest.mark.parametrize("agg", sorted(AGGS))
def test_pipeline_on_tsukuba(orc, tsukuba_gray, agg):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = tsukuba_gray
    h, w = Il.shape
    pipe = PairPipeline(w, h, 16, dminl=-15, adjust=_p(**ADJ), subpixel="parabola", **AGGS[agg])
    assert pipe.agg is not None and pipe.adjust_ws_bytes == 255 + 8 * w * h
    pipe.run(_t(Il), _t(Ir))
    got = pipe.results()
    want = _chain(orc, Il, got, -15, 16, ADJ, subpixel="parabola")
    _bits(got["occlusion"], want["occlusion"], f"{agg} occlusion")
    _bits(got["filled"], want["filled"], f"{agg} filled")
    _bits(got["adjusted"], want["filled"], f"{agg} adjusted")
    _bits(got["subpix_filled"], want["sub_filled"], f"{agg} sub_filled")
    moved = want["filled"].view(np.uint32) != want["before"].view(np.uint32)
    print(f"Tsukuba, {agg}: {int(moved.sum())} of {moved.size} pixels of the filled map change")
    assert moved.sum() > 0


@pytest.fixture(scope="module")
def pair(orc):
    rgb_l, rgb_r = cgf_ref.colour_pair(PW, PH, PD, 4711)
    return dict(Il=orc.gray(rgb_l), Ir=orc.gray(rgb_r))


def test_composition_with_uniqueness_speckle_vote_subpixel_and_weighted_median(orc, pair):
    from stereo_matching_cuda_amd.device import PairPipeline
    spk = _lib.SpeckleParams()
    spk.max_size, spk.max_diff = 30, 1.0
    vp = smx.default_vote_params()
    vp.tau_s, vp.iterations = 10, 3
    xp = smx.default_cross_params()
    xp.l1, xp.l2 = 17, 8
    vote = (dict(tau_s=10, tau_h_pct=40, iterations=3, interpolate_=1), dict(l1=17, l2=8, tau1=20, tau2=6),
            int(smx.default_params().d_lr))
    want = None
    for sif in (None, 5):
        pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="cross", cost="census", adjust=_p(**ADJ), speckle=spk,
                            uniqueness=fuzz_scenes.ratio_of(5), vote=vp, vote_arms=xp, subpixel="equiangular", wmf="occluded",
                            slices_in_flight=sif)
        pipe.run(_t(pair["Il"]), _t(pair["Ir"]))
        got = pipe.results()
        if want is None:
            want = _chain(orc, pair["Il"], got, PDMINL, PD, ADJ, subpixel="equiangular", wmf="occluded", vote=vote, uniqueness=5,
                          speckle=(30, 1.0))
        for k, name in (("occlusion",) * 2, ("unique",) * 2, ("despeckled",) * 2, ("voted",) * 2, ("filled",) * 2,
                        ("adjusted", "filled"), ("subpix_filled", "sub_filled"), ("refined",) * 2):
            _bits(got[k], want[name], f"slices in flight {sif}: {k}")
    assert (want["filled"] != want["before"]).any() and (want["voted"] != want["despeckled"]).any()


def test_adjust_none_is_byte_for_byte_a_pipeline_built_without_the_argument(orc, pair):
    from stereo_matching_cuda_amd.device import PairPipeline
    res = []
    for kw in ({}, dict(adjust=None)):
        pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, subpixel="parabola", wmf="all", **kw)
        assert pipe.adjust is None and pipe.adjusted is None and pipe.adjust_ws is None and pipe.adjust_ws_bytes == 0 and pipe.agg is None
        pipe.run(_t(pair["Il"]), _t(pair["Ir"]))
        res.append(pipe.results())
    assert sorted(res[0]) == sorted(res[1]) and "adjusted" not in res[0] and "aggl" not in res[0]
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k
    want = orc.stereo_pair(pair["Il"], pair["Ir"], PD, dminl=PDMINL, dminr=0)
    for k in ("dmapl", "dmapr", "occlusion", "filled"):
        _bits(res[0][k], want[k], k)
    true = PairPipeline(PW, PH, PD, dminl=PDMINL, adjust=True)
    assert (true.adjust.tau_e, true.adjust.vertical, true.adjust.iterations) == (2, 1, 1)


def test_pipeline_refusals():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    for kw in (dict(s_begin=1), dict(s_end=PD - 1), dict(max_ws_bytes=2 * PD * PW * PH * 4)):
        with pytest.raises(ValueError):
            PairPipeline(PW, PH, PD, adjust=True, **kw)
    with pytest.raises(ValueError, match="adjustment"):
        ShardedPair(PW, PH, PD, adjust=True)


# ---------------------------------------------------------------------------------------------
# the context
# ---------------------------------------------------------------------------------------------
def _sub_filled(ctx):
    s = np.empty((PH, PW), F32)
    _lib.check(smx.lib().smx_ctx_subpixel_maps(ctx, None, None, s.ctypes.data))
    return s


def test_context(orc, pair):
    L = smx.lib()
    ctx = _ctx_create()
    gray = (pair["Il"], pair["Ir"])
    try:
        rc, off = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, True)
        _lib.check(rc)
        plain = orc.stereo_pair(*gray, PD, dminl=PDMINL, dminr=0)
        for k, name in CTX_NAMES:
            _bits(off[k], plain[name], "off " + name)
        for bad in (dict(tau_e=0), dict(tau_e=513), dict(vertical=2), dict(iterations=0), dict(iterations=9)):
            assert L.smx_ctx_set_adjust(ctx, C.byref(_p(**bad))) == -1 and b"tau_e" in L.smx_last_error()
        rc, still = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)           # a refused setter leaves it off
        _lib.check(rc)
        _bits(still["filled"], plain["filled"], "still off")
        # on: whether the caller asks for the volumes or not
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(_p(**ADJ))))
        assert L.smx_ctx_stereo_pair_async(ctx, gray[0].ctypes.data, gray[1].ctypes.data, PDMINL, 0) == -1
        assert b"smx_ctx_set_adjust" in L.smx_last_error()
        want = ref.adjust(plain["filled"], off["agg_l"], PDMINL, **ADJ)
        assert _changed(want, plain["filled"]) > 0
        for want_vol in (False, True):
            rc, on = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, want_vol)
            _lib.check(rc)
            for k, name in CTX_NAMES[:5]:
                _bits(on[k], plain[name], "on " + name)                         # (occlusion stays the LR-check map)
            _bits(on["filled"], want, f"filled, volumes {want_vol}")
            if want_vol:
                _bits(on["agg_l"], off["agg_l"], "agg_l")
        # with the sub-pixel fit: the changed pixels of the filled sub-pixel map carry their own fits
        _lib.check(L.smx_ctx_set_adjust(ctx, None))
        _lib.check(L.smx_ctx_set_subpixel(ctx, subpix_ref.PARABOLA))
        rc, _ = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        sub_plain = _sub_filled(ctx)
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(_p(**ADJ))))
        rc, on = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        want, wsub = ref.adjust(plain["filled"], off["agg_l"], PDMINL, mode=subpix_ref.PARABOLA, sub=sub_plain, **ADJ)
        _bits(on["filled"], want, "filled with sub-pixel")
        _bits(_sub_filled(ctx), wsub, "sub_filled")
        assert (wsub.view(np.uint32) != sub_plain.view(np.uint32)).any()
        _lib.check(L.smx_ctx_set_subpixel(ctx, 0))
        # through semi-global matching
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["sgm"], None))
        _lib.check(L.smx_ctx_set_adjust(ctx, None))
        rc, sgm_off = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, True)
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(_p(**ADJ))))
        rc, sgm_on = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        _bits(sgm_on["filled"], ref.adjust(sgm_off["filled"], sgm_off["agg_l"], PDMINL, **ADJ), "filled behind SGM")
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["guided"], None))
        # off, and on again with the defaults
        _lib.check(L.smx_ctx_set_adjust(ctx, None))
        rc, again = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        for k, name in CTX_NAMES:
            _bits(again[k], plain[name], "off again " + name)
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(_p())))
        rc, on = _ctx_pair(ctx, L.smx_ctx_stereo_pair, gray, 0, False)
        _lib.check(rc)
        _bits(on["filled"], ref.adjust(plain["filled"], off["agg_l"], PDMINL), "the defaults")
    finally:
        L.smx_destroy(ctx)


def test_a_context_of_more_than_512_labels_refuses():
    L = smx.lib()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), 40, 8, 513, C.byref(ctx)))
    try:
        assert L.smx_ctx_set_adjust(ctx, C.byref(_p())) == -1 and b"size_d" in L.smx_last_error()
    finally:
        L.smx_destroy(ctx)
