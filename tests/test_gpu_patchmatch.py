"""PatchMatch stereo on the GPU (smx_dev_patchmatch_pair, smx_dev_pm_plane_cost and everything above them) against
tests/patchmatch_ref.py, bit for bit: planes, costs, disp and labels of both views compared as uint32.  Every buffer of a device
call lies in a Guarded (tests/guarded.py); the workspace is poisoned with 0xFF and misaligned by 0, 1 or 255 bytes.  A case's
reference is computed once and shared by the tests that use it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import patchmatch_ref as ref
from guarded import Guarded
from test_patchmatch_cpu import bits, default_cc, pm_params, random_pair, ref_params

pytestmark = pytest.mark.gpu

F32 = np.float32
MISALIGN = (0, 1, 255)
OUTPUTS = ("planes", "cost", "disp", "label")

# name -> w, h, radius, size_d, dminl, dminr, iterations, max_slope.  What the issue's table leaves open is the small
# configuration: radius 2, 6 labels from -5 / 0, 2 iterations, max_slope 2.
CASES = {
    "single pixel": (1, 1, 2, 6, -5, 0, 2, 2.0),
    "every +-5 neighbour outside": (6, 6, 2, 6, -5, 0, 2, 2.0),
    "odd sizes, unequal colours": (37, 19, 2, 6, -5, 0, 2, 2.0),
    "two waves of a colour in a row": (131, 6, 1, 6, -5, 0, 2, 2.0),
    "window taller than the image": (70, 9, 8, 6, -5, 0, 1, 2.0),
    "largest radius": (40, 38, 17, 6, -5, 0, 1, 2.0),
    "size_d 1": (33, 21, 2, 1, -2, 0, 2, 2.0),
    "size_d 300": (33, 21, 2, 300, -299, 0, 2, 2.0),
    "positive dmin": (33, 21, 2, 6, 3, 2, 2, 2.0),
    "max_slope 0": (33, 21, 2, 6, -5, 0, 2, 0.0),
}


def _same(got, want, name):
    for k in OUTPUTS:
        a, b = bits(got[k]).ravel(), bits(want[k]).ravel()
        assert a.shape == b.shape, (name, k)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f"{name}: {k}: {bad.size} of {a.size} values differ, first at {bad[:5]}: "
                               f"{got[k].ravel()[bad[:5]]} != {want[k].ravel()[bad[:5]]}")


def _stream(s=None):
    import torch
    return C.c_void_p((s or torch.cuda.current_stream()).cuda_stream)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (left, right, pm, the reference's outputs) of a case; read-only"""
    w, h, radius, size_d, dminl, dminr, iterations, slope = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name))
    left, right = random_pair(rng, h, w, -2 if dminl < 0 else 3)
    pm = dict(radius=radius, iterations=iterations, max_slope=slope, seed=7)
    want = ref.patchmatch(left, right, size_d, dminl, dminr, ref_params(pm_params(**pm)), default_cc())
    for a in (left, right, *want.values()):
        a.setflags(write=False)
    return left, right, pm, want


class Call:
    """The buffers of one smx_dev_patchmatch_pair / smx_dev_pm_plane_cost call, guarded"""

    def __init__(self, left, right, size_d, dminl, dminr, misalign=0, ws_bytes=None, planes=None):
        h, w = left.shape
        n = w * h
        self.shape, self.geo = (h, w), (w, h, size_d, dminl, dminr)
        self.left = Guarded(n, np.uint8, (h, w), plane=n).load(left)
        self.right = Guarded(n, np.uint8, (h, w), plane=n).load(right)
        self.planes = Guarded(24 * n, F32, (2, 3, h, w), plane=n)
        if planes is not None:
            self.planes.load(planes)
        self.out = {k: Guarded(8 * n, F32, (2, h, w), plane=n) for k in OUTPUTS[1:]}
        self.ws_bytes = int(smx.lib().smx_pm_workspace_bytes(w, h)) if ws_bytes is None else ws_bytes
        self.ws = Guarded(self.ws_bytes, np.uint8, (self.ws_bytes,), misalign=misalign, fill=0xFF, plane=n)

    def search(self, pm, stream=None):
        return smx.lib().smx_dev_patchmatch_pair(C.byref(smx.default_params()), C.byref(pm), self.left.ptr, self.right.ptr, *self.geo,
                                                 self.planes.ptr, self.out["cost"].ptr, self.out["disp"].ptr, self.out["label"].ptr,
                                                 self.ws.ptr, self.ws_bytes, _stream(stream))

    def cost(self, pm, stream=None):
        return smx.lib().smx_dev_pm_plane_cost(C.byref(smx.default_params()), C.byref(pm), self.left.ptr, self.right.ptr, *self.geo,
                                               self.planes.ptr, self.out["cost"].ptr, self.ws.ptr, self.ws_bytes, _stream(stream))

    def check_memory(self, planes_in=False):
        self.left.check_unchanged("d_left")
        self.right.check_unchanged("d_right")
        if planes_in:
            self.planes.check_unchanged("d_planes")
        else:
            self.planes.check("d_planes")
        for k, g in self.out.items():
            g.check("d_" + k)
        self.ws.check("d_ws")

    def results(self):
        r = {k: g.numpy() for k, g in self.out.items()}
        r["planes"] = self.planes.numpy()
        return r


def run_case(name, misalign=0, stream=None):
    left, right, pm, want = case(name)
    _, _, _, size_d, dminl, dminr, _, _ = CASES[name]
    c = Call(left, right, size_d, dminl, dminr, misalign)
    _lib.check(c.search(pm_params(**pm), stream))
    c.check_memory()
    return c.results(), want


# ---------------------------------------------------------------------------------------------
# the search
# ---------------------------------------------------------------------------------------------
def test_the_footprint_is_what_the_shapes_assume():
    tw, th = C.c_int(0), C.c_int(0)
    _lib.check(smx.lib().smx_pm_geometry(C.byref(tw), C.byref(th)))
    assert (tw.value, th.value) == (64, 4)      # 131 columns: 66 pixels of a colour in a row, two waves


@pytest.mark.parametrize("name", list(CASES))
def test_the_search_equals_the_reference(name):
    got, want = run_case(name, MISALIGN[list(CASES).index(name) % 3])
    _same(got, want, name)
    w, h, _, size_d, dminl, dminr, _, slope = CASES[name]
    for v, dmin in enumerate((dminl, dminr)):
        assert got["disp"][v].min() >= dmin and got["disp"][v].max() <= dmin + size_d - 1
        assert np.abs(got["planes"][v, :2]).max() <= slope


def test_run_to_run_identity_and_a_second_stream():
    import torch
    name = "odd sizes, unequal colours"
    a, want = run_case(name)
    b, _ = run_case(name, 255)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c, _ = run_case(name, 1, s)
    s.synchronize()
    for r in (a, b, c):
        _same(r, want, name)


def test_the_host_pointer_entry():
    name = "every +-5 neighbour outside"
    left, right, pm, want = case(name)
    _, _, _, size_d, dminl, dminr, _, _ = CASES[name]
    _same(smx.patchmatch(left, right, size_d, dminl, dminr, pm_params(**pm)), want, name)


def test_a_small_workspace_is_refused_before_any_launch():
    left, right, pm, _ = case("every +-5 neighbour outside")
    need = int(smx.lib().smx_pm_workspace_bytes(6, 6))
    c = Call(left, right, 6, -5, 0, ws_bytes=need - 1)
    assert c.search(pm_params(**pm)) == -3 and b"workspace" in smx.lib().smx_last_error()
    assert c.cost(pm_params(**pm)) == -3
    for g in (c.planes, c.ws, *c.out.values()):
        g.check_untouched("refused call")


# ---------------------------------------------------------------------------------------------
# the plane cost alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd sizes, unequal colours", "window taller than the image"])
def test_plane_cost_of_random_planes(name):
    left, right, pm, _ = case(name)
    w, h, _, size_d, dminl, dminr, _, _ = CASES[name]
    rng = np.random.default_rng(3)
    planes = np.empty((2, 3, h, w), F32)
    planes[:, :2] = rng.uniform(-2.5, 2.5, (2, 2, h, w))
    planes[0, 2] = rng.uniform(dminl - 1.5, dminl + size_d + 0.5, (h, w))       # some outside the labels
    planes[1, 2] = rng.uniform(dminr - 1.5, dminr + size_d + 0.5, (h, w))
    planes[0, 2, 0, 0], planes[0, 0, 1, 1], planes[1, 1, 2, 2], planes[1, 2, 3, 3] = np.nan, np.inf, -np.inf, 3e38
    cc, rp = default_cc(), ref_params(pm_params(**pm))
    want = np.stack([ref.plane_cost_map(left, right, dminl, size_d, rp, cc, planes[0]),
                     ref.plane_cost_map(right, left, dminr, size_d, rp, cc, planes[1])])
    c = Call(left, right, size_d, dminl, dminr, 1, planes=planes)
    _lib.check(c.cost(pm_params(**pm)))
    c.check_memory(planes_in=True)
    assert np.array_equal(bits(c.out["cost"].numpy()), bits(want))
    for k in ("disp", "label"):
        c.out[k].check_untouched(k)
    assert np.array_equal(bits(smx.pm_plane_cost(left, right, planes, size_d, dminl, dminr, pm_params(**pm))), bits(want))


def test_radius_0_fronto_parallel_planes_are_the_cost_volume():
    rng = np.random.default_rng(2)
    h, w, size_d, dminl, dminr = 9, 70, 8, -7, 0
    left, right = random_pair(rng, h, w, -3)
    vl, vr = oracle.cost_volume(left, right, size_d, dminl), oracle.cost_volume(right, left, size_d, dminr)
    border = int(bits(default_cc()["border"]).ravel()[0])
    pm = pm_params(radius=0)
    seen = 0
    for z in range(size_d):
        planes = np.zeros((2, 3, h, w), F32)
        planes[0, 2], planes[1, 2] = dminl + z, dminr + z
        got = bits(smx.pm_plane_cost(left, right, planes, size_d, dminl, dminr, pm))
        assert np.array_equal(got[0], bits(vl[z])) and np.array_equal(got[1], bits(vr[z])), z
        seen += int((got == border).sum())
    assert seen > 0


# ---------------------------------------------------------------------------------------------
# the context and PairPipeline
# ---------------------------------------------------------------------------------------------
PW, PH, PD, PDMINL = 48, 26, 8, -7
PPM = dict(radius=2, iterations=2, seed=5)
SPK = (12, 1.0)
PLANES = ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")


@functools.lru_cache(maxsize=None)
def pair_scene():
    """A pair whose right view is the left one moved by a block-wise disparity (so that the LR check drops pixels), the
    reference's search on it, and the plain pair of the oracle"""
    rng = np.random.default_rng(77)
    tex = rng.integers(0, 256, (PH, PW + 16)).astype(np.uint8)
    left = tex[:, 8:8 + PW].copy()
    right = left.copy()
    right[:, :PW - 2] = left[:, 2:]                     # left (x) matches right (x - 2)
    right[8:18, 10:30] = left[8:18, 15:35]              # a nearer block: x matches x - 5
    want = ref.patchmatch(left, right, PD, PDMINL, 0, ref_params(pm_params(**PPM)), default_cc())
    plain = oracle.stereo_pair(left, right, PD, dminl=PDMINL, dminr=0)
    for a in (left, right, *want.values()):
        a.setflags(write=False)
    return left, right, want, plain


def chain(speckle=False, wmf=None):
    """What the pair hands out behind the reference's search, from the existing references"""
    import speckle_ref
    import subpix_ref
    import wmf_ref
    left, _, want, _ = pair_scene()
    r = {"best_l": want["cost"][0], "best_r": want["cost"][1], "dmap_l": want["label"][0], "dmap_r": want["label"][1]}
    r["occlusion"] = oracle.detect_occlusion(r["dmap_l"], r["dmap_r"], PDMINL - 100)
    kept = r["occlusion"]
    if speckle:
        kept = r["despeckled"] = speckle_ref.speckle_filter(kept, float(PDMINL), float(PDMINL - 100), *SPK)
    r["filled"] = oracle.fill_occlusion(kept, PDMINL)
    r["sub_filled"] = np.where(subpix_ref.kept(kept, PDMINL), want["disp"][0], r["filled"]).astype(F32)
    if wmf:
        wp = smx.default_wmf_params()
        ws, wc = smx.wmf_weights(wp)
        r["refined"] = wmf_ref.weighted_median(left, r["filled"], PDMINL, PD, kept if wmf == "occluded" else None, wp.radius, ws, wc)
    return r


def _eq(got, want, name):
    assert np.array_equal(bits(got), bits(want)), f"{name}: {int((bits(got) != bits(want)).sum())} values differ"


def _ctx_pair(ctx, left, right, **extra):
    bufs = {k: np.empty((PH, PW), F32) for k in PLANES}
    bufs.update(extra)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    return smx.lib().smx_ctx_stereo_pair(ctx, left.ctypes.data, right.ctypes.data, PDMINL, 0, C.byref(out)), bufs


def _held(ctx):
    b = C.c_size_t(123)
    _lib.check(smx.lib().smx_ctx_pm_held(ctx, C.byref(b)))
    return b.value


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


def test_context():
    L = smx.lib()
    left, right, want, plain = pair_scene()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), PW, PH, PD, C.byref(ctx)))
    names = dict(best_l="bestl", best_r="bestr", dmap_l="dmapl", dmap_r="dmapr", occlusion="occlusion", filled="filled")
    n = PW * PH
    maps = [np.empty((3, PH, PW), F32), np.empty((3, PH, PW), F32)] + [np.empty((PH, PW), F32) for _ in range(3)]
    ptrs = [m.ctypes.data for m in maps]
    try:
        # off by default: the plain pair, nothing held, no maps
        rc, off = _ctx_pair(ctx, left, right)
        _lib.check(rc)
        for k in PLANES:
            _eq(off[k], plain[names[k]], "off " + k)
        assert _held(ctx) == 0
        assert L.smx_ctx_patchmatch_maps(ctx, *ptrs) == -1 and b"without PatchMatch" in L.smx_last_error()
        # a refused setter leaves it off
        for bad in (dict(radius=18), dict(gamma=0.0), dict(iterations=0), dict(max_slope=9.0)):
            assert L.smx_ctx_set_patchmatch(ctx, C.byref(pm_params(**bad))) == -1 and b"radius" in L.smx_last_error()
        rc, still = _ctx_pair(ctx, left, right)
        _lib.check(rc)
        _eq(still["filled"], plain["filled"], "still off")
        assert _held(ctx) == 0
        # on
        _lib.check(L.smx_ctx_set_patchmatch(ctx, C.byref(pm_params(**PPM))))
        assert _held(ctx) == 0                                   # (allocated by the first pair, not by the setter)
        rc, on = _ctx_pair(ctx, left, right)
        _lib.check(rc)
        w = chain()
        for k in PLANES:
            _eq(on[k], w[k], "on " + k)
        assert (bits(w["occlusion"]) != bits(w["dmap_l"])).any()          # the LR check dropped pixels
        assert _held(ctx) == 8 * n * 4 + L.smx_pm_workspace_bytes(PW, PH)
        _lib.check(L.smx_ctx_patchmatch_maps(ctx, *ptrs))
        _eq(maps[0], want["planes"][0], "planes_l")
        _eq(maps[1], want["planes"][1], "planes_r")
        _eq(maps[2], want["disp"][0], "sub_l")
        _eq(maps[3], want["disp"][1], "sub_r")
        _eq(maps[4], w["sub_filled"], "sub_filled")
        assert (bits(w["sub_filled"]) != bits(want["disp"][0])).any() and (bits(w["sub_filled"]) != bits(w["filled"])).any()
        _lib.check(L.smx_ctx_patchmatch_maps(ctx, None, None, None, None, None))
        # with speckle removal behind the LR check
        _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk())))
        rc, on = _ctx_pair(ctx, left, right)
        _lib.check(rc)
        ws = chain(speckle=True)
        for k in PLANES:
            _eq(on[k], ws[k], "speckle " + k)
        desp = np.empty((PH, PW), F32)
        _lib.check(L.smx_ctx_speckle_map(ctx, desp.ctypes.data))
        _eq(desp, ws["despeckled"], "despeckled")
        _lib.check(L.smx_ctx_patchmatch_maps(ctx, None, None, None, None, ptrs[4]))
        _eq(maps[4], ws["sub_filled"], "sub_filled behind speckle removal")
        assert (bits(ws["despeckled"]) != bits(ws["occlusion"])).any()
        _lib.check(L.smx_ctx_set_speckle(ctx, None))
        # every refused combination
        vol = np.empty((PD, PH, PW), F32)
        u8 = np.empty((PH, PW), np.uint8)
        for extra in (dict(cost_l=vol), dict(cost_r=vol), dict(agg_l=vol), dict(agg_r=vol), dict(mean_l=u8), dict(mean_r=u8)):
            rc, _ = _ctx_pair(ctx, left, right, **extra)
            assert rc == -1 and b"smx_ctx_set_patchmatch" in L.smx_last_error(), extra
        assert L.smx_ctx_stereo_pair_async(ctx, left.ctypes.data, right.ctypes.data, PDMINL, 0) == -1
        assert b"smx_ctx_set_patchmatch" in L.smx_last_error()
        toggles = (
            ("census", lambda: L.smx_ctx_set_cost(ctx, _lib.COST_MODES["census"], None),
             lambda: L.smx_ctx_set_cost(ctx, _lib.COST_MODES["reference"], None)),
            ("adcensus", lambda: L.smx_ctx_set_adcensus(ctx, C.byref(smx.default_adcensus_params())),
             lambda: L.smx_ctx_set_adcensus(ctx, None)),
            ("rgb guide", lambda: L.smx_ctx_set_guidance(ctx, _lib.GUIDE_MODES["rgb"]),
             lambda: L.smx_ctx_set_guidance(ctx, _lib.GUIDE_MODES["gray"])),
            ("sgm", lambda: L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["sgm"], None),
             lambda: L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["guided"], None)),
            ("cross", lambda: L.smx_ctx_set_cross(ctx, C.byref(smx.default_cross_params())), lambda: L.smx_ctx_set_cross(ctx, None)),
            ("scanline", lambda: L.smx_ctx_set_scanline(ctx, C.byref(smx.default_scanline_params())),
             lambda: L.smx_ctx_set_scanline(ctx, None)),
            ("cross-scale", lambda: L.smx_ctx_set_cross_scale(ctx, C.byref(smx.default_cscale_params())),
             lambda: L.smx_ctx_set_cross_scale(ctx, None)),
            ("adjust", lambda: L.smx_ctx_set_adjust(ctx, C.byref(smx.default_adjust_params())), lambda: L.smx_ctx_set_adjust(ctx, None)),
            ("uniqueness", lambda: L.smx_ctx_set_uniqueness(ctx, 0.15), lambda: L.smx_ctx_set_uniqueness(ctx, 0.0)),
            ("subpixel", lambda: L.smx_ctx_set_subpixel(ctx, 1), lambda: L.smx_ctx_set_subpixel(ctx, 0)),
        )
        for name, on_, off_ in toggles:
            _lib.check(on_())
            rc, _ = _ctx_pair(ctx, left, right)
            assert rc == -1 and L.smx_last_error(), name
            _lib.check(off_())
        # off again: the plain pair, bit for bit
        _lib.check(L.smx_ctx_set_patchmatch(ctx, None))
        rc, again = _ctx_pair(ctx, left, right)
        _lib.check(rc)
        for k in PLANES:
            _eq(again[k], plain[names[k]], "off again " + k)
        assert L.smx_ctx_patchmatch_maps(ctx, *ptrs) == -1
    finally:
        L.smx_destroy(ctx)


def test_context_colour_entry():
    """smx_ctx_stereo_pair_rgb with PatchMatch on: the search runs on the gray images the entry makes on the device"""
    L = smx.lib()
    left, right, _, _ = pair_scene()
    rgb = [np.ascontiguousarray(np.stack([g, g[:, ::-1], g[::-1]], axis=2)) for g in (left, right)]
    gl, gr = oracle.gray(rgb[0]), oracle.gray(rgb[1])
    want = ref.patchmatch(gl, gr, PD, PDMINL, 0, ref_params(pm_params(**PPM)), default_cc())
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), PW, PH, PD, C.byref(ctx)))
    try:
        _lib.check(L.smx_ctx_set_patchmatch(ctx, C.byref(pm_params(**PPM))))
        bufs = {k: np.empty((PH, PW), F32) for k in PLANES}
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        _lib.check(L.smx_ctx_stereo_pair_rgb(ctx, rgb[0].ctypes.data, rgb[1].ctypes.data, 3, PDMINL, 0, C.byref(out)))
        for k, w in (("best_l", want["cost"][0]), ("best_r", want["cost"][1]), ("dmap_l", want["label"][0]),
                     ("dmap_r", want["label"][1])):
            _eq(bufs[k], w, "colour entry " + k)
        _eq(bufs["occlusion"], oracle.detect_occlusion(want["label"][0], want["label"][1], PDMINL - 100), "colour entry occlusion")
        planes = np.empty((3, PH, PW), F32)
        _lib.check(L.smx_ctx_patchmatch_maps(ctx, planes.ctypes.data, None, None, None, None))
        _eq(planes, want["planes"][0], "colour entry planes_l")
    finally:
        L.smx_destroy(ctx)


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()         # (a copy: the scene's arrays are read-only)


@pytest.mark.parametrize("speckle,wmf", [(False, None), (True, "occluded"), (False, "all")])
def test_pair_pipeline(speckle, wmf):
    from stereo_matching_cuda_amd.device import PairPipeline
    left, right, want, _ = pair_scene()
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="patchmatch", pm_params=pm_params(**PPM),
                        speckle=_spk() if speckle else None, wmf=wmf)
    pipe.run(_t(left), _t(right))
    got = pipe.results()
    w = chain(speckle, wmf)
    for k, name in (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"), ("occlusion", "occlusion"),
                    ("filled", "filled")):
        _eq(got[name], w[k], name)
    _eq(got["pm_planes"], want["planes"], "planes")
    _eq(got["subpixl"], want["disp"][0], "disp_l")
    _eq(got["subpixr"], want["disp"][1], "disp_r")
    _eq(got["subpix_filled"], w["sub_filled"], "sub_filled")
    if speckle:
        _eq(got["despeckled"], w["despeckled"], "despeckled")
    if wmf:
        _eq(got["refined"], w["refined"], "refined")
        assert (bits(w["refined"]) != bits(w["filled"])).any()
    assert not got["meanl"].any()


def test_pair_pipeline_refusals():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    pm = dict(aggregation="patchmatch")
    for kw in (dict(cost="census"), dict(cost="adcensus"), dict(guidance="rgb"), dict(cross_scale=True), dict(adjust=True),
               dict(uniqueness=0.15), dict(subpixel="parabola"), dict(want_agg=True), dict(s_begin=1), dict(s_end=PD - 1),
               dict(pm_params=pm_params(radius=18)), dict(pm_params=pm_params(iterations=0)), dict(pm_params=pm_params(gamma=0.0)),
               dict(pm_params=pm_params(max_slope=8.5)), dict(pm_params="defaults")):
        with pytest.raises(ValueError):
            PairPipeline(PW, PH, PD, dminl=PDMINL, **pm, **kw)
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, dminl=PDMINL, pm_params=pm_params())               # pm_params without the aggregation
    with pytest.raises(ValueError):
        PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation="patch-match")
    for agg in ("sgm", "cross", "scanline", "cross-scanline"):                          # one aggregation at a time
        with pytest.raises(ValueError):
            PairPipeline(PW, PH, PD, dminl=PDMINL, aggregation=agg, pm_params=pm_params())
    with pytest.raises(ValueError, match="PatchMatch"):
        ShardedPair(PW, PH, PD, **pm)
    left, right, _, _ = pair_scene()
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL, **pm)
    vol = _t(np.zeros((PD, PH, PW), F32))
    with pytest.raises(ValueError):
        pipe.aggregate(_t(left), _t(right), vol, vol)


def test_a_pipeline_without_it_is_the_plain_pair():
    from stereo_matching_cuda_amd.device import PairPipeline
    left, right, _, plain = pair_scene()
    pipe = PairPipeline(PW, PH, PD, dminl=PDMINL)
    assert pipe.pm_planes is None and pipe.pm_ws is None and pipe.pm_ws_bytes == 0 and pipe.sub_filled is None
    pipe.run(_t(left), _t(right))
    got = pipe.results()
    for k in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled"):
        _eq(got[k], plain[k], k)
    assert "pm_planes" not in got
