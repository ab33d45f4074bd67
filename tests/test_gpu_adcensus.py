"""The AD-Census matching cost on the GPU (smx_dev_adcensus_cost_pair, smx_adcensus_cost, PairPipeline(cost="adcensus"),
smx_ctx_set_adcensus).  The kernel is held to tests/adcensus_ref.py bit for bit, with its outputs inside guard bands
(tests/guarded.py); everything behind it to the oracle or the numpy references fed with the reference's volume.  All
comparisons are equality of the bit patterns.

k_adcensus_cost_pair works on 256 columns x 16 slices: the shapes aim at those edges.

Run on the GPU box:  python -m pytest tests -m gpu -q -k adcensus
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import adcensus_ref as ref
import census_ref
import cgf_ref
import sgm_ref
import speckle_ref
import subpix_ref
import uniq_ref
import wmf_ref
from guarded import Guarded
from test_gpu_census import MAPS, PAIRS, _codes, _dp, _eq, _rand_pair, _stream

pytestmark = pytest.mark.gpu


def _ap(colour=0, rx=4, ry=3, th=62, lc=30.0, la=10.0, scale=127.5):
    p = _lib.AdCensusParams()
    p.census.rx, p.census.ry, p.census.th = rx, ry, th
    p.lambda_census, p.lambda_ad, p.scale, p.colour = lc, la, scale, colour
    return p


def _kw(p):
    """the parameters as the keywords of adcensus_ref.cost"""
    return dict(rx=p.census.rx, ry=p.census.ry, th=p.census.th, lambda_census=p.lambda_census, lambda_ad=p.lambda_ad,
                scale=p.scale, colour=p.colour)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _table(p):
    import torch
    tab = torch.empty(_lib.ADCENSUS_TABLE_FLOATS, dtype=torch.float32, device="cuda")
    _lib.check(smx.lib().smx_dev_adcensus_tables(C.byref(p), _dp(tab), _stream()))
    return tab


def _images(w, h, seed, ch):
    """(the images of the AD term, the gray images of the codes) of a random pair: with ch == 1 the same arrays; else random
    colour images -- a 4th byte random too -- beside gray images of their own (the kernel takes the codes as they come)."""
    gl, gr = _rand_pair(w, h, seed)
    if ch == 1:
        return (gl, gr), (gl, gr)
    rng = np.random.default_rng(seed + 1000)
    return tuple(rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8) for _ in range(2)), (gl, gr)


def _cost_pair(p, imgs, grays, dminl, dminr, s0, s1, left=True, right=True, misalign=0):
    """smx_dev_adcensus_cost_pair on guarded outputs -> (left volume or None, right volume or None) as numpy."""
    h, w = grays[0].shape
    ch = 1 if imgs[0].ndim == 2 else imgs[0].shape[2]
    codes = _codes(grays[0], grays[1], p.census)
    tab, il, ir = _table(p), _t(imgs[0]), _t(imgs[1])
    shape = (s1 - s0, h, w)
    out = [Guarded((s1 - s0) * h * w * 4, np.float32, shape, misalign=misalign, plane=w * h) if on else None
           for on in (left, right)]
    ptr = [g.ptr if g is not None else None for g in out]
    _lib.check(smx.lib().smx_dev_adcensus_cost_pair(C.byref(p), _dp(tab), _dp(codes), _dp(il), _dp(ir), ch, ptr[0], ptr[1], w, h,
                                                    dminl, dminr, s0, s1, _stream()))
    res = []
    for name, g in zip(("left", "right"), out):
        if g is None:
            res.append(None)
            continue
        if s1 == s0:
            g.check_untouched(name)
            res.append(np.empty(shape, np.float32))
        else:
            g.check(name)
            res.append(g.numpy())
    return res


def _want(p, imgs, grays, D, dminl, dminr, s0=0, s1=None):
    kw = _kw(p)
    return (ref.cost(imgs[0], imgs[1], grays[0], grays[1], D, dminl, s_begin=s0, s_end=s1, **kw),
            ref.cost(imgs[1], imgs[0], grays[1], grays[0], D, dminr, s_begin=s0, s_end=s1, **kw))


def _border(p):
    t = ref.tables(p.lambda_census, p.lambda_ad, p.scale, p.colour)
    return t[min(p.census.th, census_ref.nbits(p.census.rx, p.census.ry))] + t[64 + 255 * (3 if p.colour else 1)]


# ---------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [1, 3, 4])
@pytest.mark.parametrize("w", [1, 97, 255, 256, 257])
def test_cost_at_the_column_edges_of_a_workgroup(w, ch):
    """One lane, and both sides of the 256-column edge, for 1, 3 and 9 rows."""
    p = _ap(colour=int(ch != 1), rx=4, ry=1, th=30)
    for h in (1, 3, 9):
        imgs, grays = _images(w, h, w + h, ch)
        cl, cr = _cost_pair(p, imgs, grays, -5, -6, 0, 12, misalign=4 * (h % 3))
        wl, wr = _want(p, imgs, grays, 12, -5, -6)
        _eq(cl, wl, f"left h {h}")
        _eq(cr, wr, f"right h {h}")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("dmin,D", [(-69, 70), (-5, 12), (3, 4), (-2, 1), (-200, 3), (150, 2)])
def test_cost_ranges(dmin, D, ch):
    """Labels left of zero, right of it, across it, one slice, and ranges that lie outside the image altogether."""
    p = _ap(colour=int(ch != 1))
    imgs, grays = _images(97, 5, D, ch)
    dminr = -(dmin + D - 1)
    cl, cr = _cost_pair(p, imgs, grays, dmin, dminr, 0, D)
    wl, wr = _want(p, imgs, grays, D, dmin, dminr)
    _eq(cl, wl, "left")
    _eq(cr, wr, "right")
    if abs(dmin) >= 150:
        assert np.all(cl.view(np.uint32) == _border(p).view(np.uint32)) and np.all(cr == _border(p))
    else:
        assert len(np.unique(cl)) > 10


@pytest.mark.parametrize("ch", [1, 4])
@pytest.mark.parametrize("s0,s1", [(0, 1), (3, 20), (16, 49), (15, 17), (69, 70), (5, 5)])
def test_cost_slice_ranges(s0, s1, ch):
    """Sub-ranges whose length is no multiple of the 16 slices of a workgroup; an empty one launches nothing."""
    p = _ap(colour=int(ch != 1), rx=2, ry=3, th=20)
    imgs, grays = _images(70, 4, 9, ch)
    cl, cr = _cost_pair(p, imgs, grays, -69, 0, s0, s1)
    wl, wr = _want(p, imgs, grays, 70, -69, 0, s0, s1)
    _eq(cl, wl, "left")
    _eq(cr, wr, "right")


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("rx,ry", [(1, 1), (4, 3)])
def test_cost_windows_and_truncation(rx, ry, ch):
    nb = census_ref.nbits(rx, ry)
    imgs, grays = _images(67, 9, rx, ch)
    for th in (1, nb, nb + 10):
        p = _ap(colour=int(ch != 1), rx=rx, ry=ry, th=th, lc=7.0, la=3.5, scale=2.0 ** 20)
        cl, cr = _cost_pair(p, imgs, grays, -4, -1, 0, 6)
        wl, wr = _want(p, imgs, grays, 6, -4, -1)
        _eq(cl, wl, f"left th {th}")
        _eq(cr, wr, f"right th {th}")
        assert cl.max() == _border(p)


def test_the_fourth_byte_does_not_matter():
    p = _ap(colour=1)
    imgs, grays = _images(131, 7, 5, 4)
    a = _cost_pair(p, imgs, grays, -17, 2, 0, 19)
    other = tuple(np.concatenate((x[..., :3], 255 - x[..., 3:]), axis=2) for x in imgs)
    b = _cost_pair(p, other, grays, -17, 2, 0, 19)
    three = tuple(np.ascontiguousarray(x[..., :3]) for x in imgs)
    c = _cost_pair(p, three, grays, -17, 2, 0, 19)
    for v in range(2):
        _eq(b[v], a[v], "another fourth byte")
        _eq(c[v], a[v], "three channels")


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_single_view_forms_and_the_host_entry(orc, ch):
    p = _ap(colour=int(ch != 1), th=40)
    imgs, _ = _images(131, 7, 1, ch)
    # the host entry makes its own gray images from colour input: the kernel gets the same ones here
    grays = imgs if ch == 1 else tuple(orc.gray(np.ascontiguousarray(x[..., :3])) for x in imgs)
    both = _cost_pair(p, imgs, grays, -17, 2, 0, 19)
    left, none = _cost_pair(p, imgs, grays, -17, 2, 0, 19, right=False)
    none2, right = _cost_pair(p, imgs, grays, -17, 2, 0, 19, left=False)
    assert none is None and none2 is None
    _eq(left, both[0], "left alone")
    _eq(right, both[1], "right alone")
    _eq(smx.adcensus_cost(imgs[0], imgs[1], 19, -17, p), both[0], "host entry, left")
    _eq(smx.adcensus_cost(imgs[1], imgs[0], 19, 2, p), both[1], "host entry, right")
    wl, wr = _want(p, imgs, grays, 19, -17, 2)
    _eq(both[0], wl, "reference, left")
    _eq(both[1], wr, "reference, right")


# ---------------------------------------------------------------------------------------------
# end to end: the pipeline against the oracle fed with the reference's volumes
# ---------------------------------------------------------------------------------------------
_EXPECTED = {}


def _oracle_params(orc, radius):
    P = orc.Params()
    smxp = smx.default_params()
    for f, _ in orc.Params._fields_:
        setattr(P, f, getattr(smxp, f))
    P.radius = radius
    return P


def _finish(orc, e, dminl):
    e["occlusion"] = orc.detect_occlusion(e["dmapl"], e["dmapr"], dminl - 100)
    e["filled"] = orc.fill_occlusion(e["occlusion"], float(dminl))
    return e


def expected(orc, Il, Ir, D, dminl, dminr, radius=9, costs=None, tag=None):
    """The maps of a pair as test_gpu_census.expected builds them, from the AD-Census volumes (costs: the two volumes, else
    the default gray ones): cost -> oracle.guided_filter for both views -> detect_occlusion -> fill_occlusion."""
    key = (tag, D, dminl, dminr, radius)
    if tag is None or key not in _EXPECTED:
        P = _oracle_params(orc, radius)
        cl, cr = costs if costs is not None else (ref.gray_cost(Il, Ir, D, dminl), ref.gray_cost(Ir, Il, D, dminr))
        bl, ml, meanl, aggl = orc.guided_filter(Il, cl, dminl, want_agg=True, params=P)
        br, mr, meanr, aggr = orc.guided_filter(Ir, cr, dminr, want_agg=True, params=P)
        e = _finish(orc, dict(costl=cl, costr=cr, bestl=bl, bestr=br, dmapl=ml, dmapr=mr, meanl=meanl, meanr=meanr, aggl=aggl,
                              aggr=aggr), dminl)
        if tag is None:
            return e
        _EXPECTED[key] = e
    return _EXPECTED[key]


def _pipe(Il, Ir, D, radius=9, ap=None, rgb=None, run=True, **kw):
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    p = smx.default_params()
    p.radius = radius
    pipe = PairPipeline(w, h, D, params=p, cost="adcensus", adcensus_params=ap, **kw)
    if run:
        imgs = _t(np.stack([Il, Ir]))
        if rgb is not None:
            pipe.run(imgs[0], imgs[1], rgb_l=_t(rgb[0]), rgb_r=_t(rgb[1]))
        else:
            pipe.run(imgs[0], imgs[1])
    return pipe


@pytest.mark.parametrize("radius,path", [(9, 5), (3, 2), (12, 1)])
@pytest.mark.parametrize("shape", sorted(PAIRS))
def test_pipeline_against_the_oracle(orc, shape, radius, path):
    w, h, D = PAIRS[shape]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, radius, tag=shape)
    pipe = _pipe(Il, Ir, D, radius, want_agg=True)
    assert smx.lib().smx_last_agg_path() == path
    r = pipe.results()
    for k in MAPS + ("aggl", "aggr"):
        _eq(r[k], e[k], f"{shape} radius {radius} {k}")
    assert len(np.unique(e["dmapl"])) > 3 and (e["occlusion"] == -(D - 1) - 100).any()
    if radius == 9:            # +0 or normal numbers in [2^-60, 2^60]: the comb walker's check never fires
        rr = C.c_int(-1)
        _lib.check(smx.lib().smx_dev_agg_fallback(_dp(pipe.ws), C.byref(rr)))
        assert rr.value == 0


def test_chunked_equals_unchunked(orc):
    w, h, D = PAIRS["129x70"]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    whole = _pipe(Il, Ir, D, want_agg=True)
    assert whole.slices_in_flight == D and whole.census_cost.shape == (2, D, h, w)
    pipe = _pipe(Il, Ir, D, slices_in_flight=5, want_agg=True)
    assert pipe.slices_in_flight == 5 and pipe.census_cost.shape == (2, 5, h, w)
    r, rw = pipe.results(), whole.results()
    for k in MAPS + ("aggl", "aggr"):
        _eq(r[k], rw[k], f"chunked against unchunked {k}")
        _eq(r[k], e[k], f"chunked {k}")
    _eq(pipe.keys.cpu().numpy(), whole.keys.cpu().numpy(), "keys")
    # a byte bound halves the slices in flight, the chunk buffer counted
    fits = 2 * smx.lib().smx_agg_workspace_bytes_for(C.byref(smx.default_params()), w, h, D) + 2 * D * w * h * 4
    assert _pipe(Il, Ir, D, run=False, max_ws_bytes=fits).slices_in_flight == D
    assert _pipe(Il, Ir, D, run=False, max_ws_bytes=fits - 1).slices_in_flight == (D + 1) // 2


# the later stages from the aggregated volumes of both views, in numpy
PW, PH, PD, PDMINL = 129, 70, 16, -15
SPK = (30, 1.0)
RATIO = 0.15
ALL_STAGES = dict(subpixel="parabola", uniqueness=RATIO, wmf="occluded", want_agg=True)
CHAIN_KEYS = ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "unique", "margin", "despeckled", "filled",
              "subpixl", "subpixr", "subpix_filled", "refined")


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = SPK
    return s


def chain(orc, Il, aggl, aggr, D, dminl, ratio=RATIO):
    r = {"aggl": aggl, "aggr": aggr}
    sl, sr = cgf_ref.states(aggl), cgf_ref.states(aggr)
    r["keys"] = np.stack((sl["keys"], sr["keys"]))
    r["bestl"], r["bestr"] = sl["best"], sr["best"]
    r["dmapl"], r["dmapr"] = subpix_ref.dmap_of(sl["z"], sl["best"], dminl), subpix_ref.dmap_of(sr["z"], sr["best"], 0)
    r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], dminl - 100)
    r["unique"], r["margin"] = uniq_ref.apply(r["occlusion"], sl["z"] >= 0, sl["best"], sl["uq"][0], ratio, dminl, dminl - 100)
    r["despeckled"] = speckle_ref.speckle_filter(r["unique"], float(dminl), float(dminl - 100), *SPK)
    r["filled"] = orc.fill_occlusion(r["despeckled"], dminl)
    mode = subpix_ref.MODES["parabola"]
    r["subpixl"], r["subpix_filled"] = subpix_ref.maps(mode, sl["z"], sl["best"], sl["nbr"][0], sl["nbr"][1], r["dmapl"],
                                                       r["despeckled"], r["filled"], dminl)
    r["subpixr"], _ = subpix_ref.maps(mode, sr["z"], sr["best"], sr["nbr"][0], sr["nbr"][1], r["dmapr"])
    wp = smx.default_wmf_params()
    ws, wc = smx.wmf_weights(wp)
    r["refined"] = wmf_ref.weighted_median(Il, r["filled"], dminl, D, r["despeckled"], wp.radius, ws, wc)
    return r


@pytest.fixture(scope="module")
def colour_scene(orc):
    """A colour pair, its gray images and its colour AD-Census volumes (defaults, colour 1)."""
    rgb_l, rgb_r = cgf_ref.colour_pair(PW, PH, PD, 4711)
    Il, Ir = orc.gray(rgb_l), orc.gray(rgb_r)
    kw = _kw(_ap(colour=1))
    return dict(rgb=(rgb_l, rgb_r), Il=Il, Ir=Ir, costl=ref.cost(rgb_l, rgb_r, Il, Ir, PD, PDMINL, **kw),
                costr=ref.cost(rgb_r, rgb_l, Ir, Il, PD, 0, **kw))


def test_composition_with_subpixel_uniqueness_speckle_and_weighted_median(orc):
    w, h, D = PAIRS["129x70"]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    want = chain(orc, Il, e["aggl"], e["aggr"], D, -(D - 1))
    pipe = _pipe(Il, Ir, D, speckle=_spk(), slices_in_flight=16, **ALL_STAGES)
    got = pipe.results()
    for k in CHAIN_KEYS:
        _eq(got[k], want[k], k)
    _eq(pipe.keys.cpu().numpy(), want["keys"], "keys")
    assert np.any(want["unique"] != want["occlusion"]) and np.any(want["refined"] != want["filled"])
    assert np.any(want["subpixl"] != want["dmapl"])


@pytest.fixture(scope="module")
def colour_chain(orc, colour_scene):
    """cgf_ref on the colour AD-Census volumes, and the later stages from its aggregated volumes."""
    s = colour_scene
    return chain(orc, s["Il"], cgf_ref.aggregate(s["rgb"][0], s["costl"]), cgf_ref.aggregate(s["rgb"][1], s["costr"]), PD, PDMINL)


@pytest.mark.parametrize("sif", [None, 5])
def test_colour_cost_with_the_colour_guide(colour_scene, colour_chain, sif):
    s, want = colour_scene, colour_chain
    pipe = _pipe(s["Il"], s["Ir"], PD, ap=_ap(colour=1), rgb=s["rgb"], dminl=PDMINL, guidance="rgb", speckle=_spk(),
                 slices_in_flight=sif, **ALL_STAGES)
    assert pipe.cgf_ws is not None and pipe.ws_bytes == 0 and pipe.slices_in_flight == (PD if sif is None else sif)
    got = pipe.results()
    for k in CHAIN_KEYS:
        _eq(got[k], want[k], k)
    _eq(pipe.keys.cpu().numpy(), want["keys"], "keys")


def test_colour_cost_with_the_gray_guide(orc, colour_scene):
    """The one case in which a pipeline without guidance="rgb" takes rgb_l= / rgb_r=; every other pipeline refuses them."""
    from stereo_matching_cuda_amd.device import PairPipeline
    s = colour_scene
    e = expected(orc, s["Il"], s["Ir"], PD, PDMINL, 0, 9, costs=(s["costl"], s["costr"]), tag="colour")
    pipe = _pipe(s["Il"], s["Ir"], PD, ap=_ap(colour=1), rgb=s["rgb"], dminl=PDMINL, want_agg=True)
    r = pipe.results()
    for k in MAPS + ("aggl", "aggr"):
        _eq(r[k], e[k], k)
    gray = expected(orc, s["Il"], s["Ir"], PD, PDMINL, 0, 9)
    assert np.any(gray["costl"] != e["costl"])
    Il, Ir, rl, rr = _t(s["Il"]), _t(s["Ir"]), _t(s["rgb"][0]), _t(s["rgb"][1])
    with pytest.raises(ValueError):
        pipe.run(Il, Ir)                                               # the colour images are missing
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=rl)
    with pytest.raises(ValueError):
        pipe.aggregate(Il, Ir, rgb_l=rl, rgb_r=rr[:, :, 0])
    for kw in (dict(cost="adcensus"), dict(cost="census"), {}):        # gray AD term, census, the reference's cost: refused as ever
        with pytest.raises(ValueError):
            PairPipeline(PW, PH, PD, dminl=PDMINL, **kw).aggregate(Il, Ir, rgb_l=rl, rgb_r=rr)


@pytest.mark.parametrize("colour", [0, 1])
def test_semi_global_matching(orc, colour_scene, colour):
    """The float costs go through SGM's clamp to 0 .. 255, as its contract says (sgm_ref.outputs applies it)."""
    s = colour_scene
    if colour:
        cl, cr = s["costl"], s["costr"]
    else:
        cl, cr = ref.gray_cost(s["Il"], s["Ir"], PD, PDMINL), ref.gray_cost(s["Ir"], s["Il"], PD, 0)
    sl, sr = sgm_ref.outputs(cl), sgm_ref.outputs(cr)
    e = _finish(orc, dict(aggl=sl["agg"], aggr=sr["agg"], bestl=sl["best"], bestr=sr["best"],
                          dmapl=(PDMINL + sl["z"]).astype(np.float32), dmapr=sr["z"].astype(np.float32)), PDMINL)
    pipe = _pipe(s["Il"], s["Ir"], PD, ap=_ap(colour=colour), rgb=s["rgb"] if colour else None, dminl=PDMINL, aggregation="sgm",
                 want_agg=True)
    assert pipe.sgm_cost is not None and pipe.census_cost is None
    r = pipe.results()
    for k in ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled"):
        _eq(r[k], e[k], f"colour {colour} {k}")
    _eq(pipe.sgm_cost.cpu().numpy(), np.stack((cl, cr)), "the whole volumes")
    assert np.any(cl != np.floor(cl))                                  # fractions: the clamp's truncation is at work


# ---------------------------------------------------------------------------------------------
# the context
# ---------------------------------------------------------------------------------------------
NAMES = {"best_l": "bestl", "best_r": "bestr", "dmap_l": "dmapl", "dmap_r": "dmapr", "occlusion": "occlusion",
         "filled": "filled", "mean_l": "meanl", "mean_r": "meanr", "cost_l": "costl", "cost_r": "costr", "agg_l": "aggl",
         "agg_r": "aggr"}


def _ctx_run(ctx, e, fields, imgs, channels, dminl):
    L = smx.lib()
    bufs = {k: np.empty(e[NAMES[k]].shape, e[NAMES[k]].dtype) for k in fields}
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    if channels:
        rc = L.smx_ctx_stereo_pair_rgb(ctx, imgs[0].ctypes.data, imgs[1].ctypes.data, channels, dminl, 0, C.byref(out))
    else:
        rc = L.smx_ctx_stereo_pair(ctx, imgs[0].ctypes.data, imgs[1].ctypes.data, dminl, 0, C.byref(out))
    return rc, bufs


def test_context_gray(orc):
    w, h, D = PAIRS["129x70"]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    plain = orc.stereo_pair(Il, Ir, D, want_cost=True)
    L = smx.lib()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), w, h, D, C.byref(ctx)))
    maps = [k for k in NAMES if not k.startswith(("cost", "agg"))]
    try:
        for bad in (_ap(lc=0.0), _ap(la=float("nan")), _ap(scale=2.0 ** 21), _ap(colour=2), _ap(rx=5)):
            assert L.smx_ctx_set_adcensus(ctx, C.byref(bad)) == -1
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(_ap())))
        assert L.smx_ctx_set_cost(ctx, 2, None) == -1                       # still no mode of smx_ctx_set_cost
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -(D - 1), 0) == -1
        assert b"smx_ctx_set_adcensus" in L.smx_last_error()
        for fields in (maps, list(NAMES)):                                  # through the chunk buffer, then with the whole volumes
            rc, bufs = _ctx_run(ctx, e, fields, (Il, Ir), 0, -(D - 1))
            _lib.check(rc)
            for k, v in bufs.items():
                _eq(v, e[NAMES[k]], f"ctx {k}")
        # other parameters: the table is uploaded again
        p2 = _ap(rx=2, ry=1, th=9, lc=12.0, la=25.0, scale=40.0)
        kw = _kw(p2)
        e2 = expected(orc, Il, Ir, D, -(D - 1), 0, 9,
                      costs=(ref.cost(Il, Ir, Il, Ir, D, -(D - 1), **kw), ref.cost(Ir, Il, Ir, Il, D, 0, **kw)))
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(p2)))
        rc, bufs = _ctx_run(ctx, e2, maps + ["cost_l"], (Il, Ir), 0, -(D - 1))
        _lib.check(rc)
        for k, v in bufs.items():
            _eq(v, e2[NAMES[k]], f"other parameters, ctx {k}")
        # off again: the reference's maps, bit for bit, and the pipelined entry works
        _lib.check(L.smx_ctx_set_adcensus(ctx, None))
        rc, bufs = _ctx_run(ctx, plain, maps + ["cost_l", "cost_r"], (Il, Ir), 0, -(D - 1))
        _lib.check(rc)
        for k, v in bufs.items():
            _eq(v, plain[NAMES[k]], f"reference ctx {k}")
        _lib.check(L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -(D - 1), 0))
        _lib.check(L.smx_ctx_wait(ctx, None, None))
        # a later smx_ctx_set_cost switches it off as well, and it replaces the census cost
        _lib.check(L.smx_ctx_set_cost(ctx, 1, None))
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(_ap())))
        rc, bufs = _ctx_run(ctx, e, maps, (Il, Ir), 0, -(D - 1))
        _lib.check(rc)
        _eq(bufs["filled"], e["filled"], "AD-Census replaces census")
        _lib.check(L.smx_ctx_set_cost(ctx, 0, None))
        rc, bufs = _ctx_run(ctx, plain, maps, (Il, Ir), 0, -(D - 1))
        _lib.check(rc)
        for k, v in bufs.items():
            _eq(v, plain[NAMES[k]], f"after smx_ctx_set_cost {k}")
    finally:
        L.smx_destroy(ctx)


def test_context_colour(orc, colour_scene, colour_chain):
    s = colour_scene
    rgb_l, rgb_r = s["rgb"]
    e = expected(orc, s["Il"], s["Ir"], PD, PDMINL, 0, 9, costs=(s["costl"], s["costr"]), tag="colour")
    gray = expected(orc, s["Il"], s["Ir"], PD, PDMINL, 0, 9, tag="colour scene, gray AD")
    L = smx.lib()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), PW, PH, PD, C.byref(ctx)))
    fields = [k for k in NAMES if not k.startswith("mean")]
    try:
        # colour 0 through the rgb entry: the AD term from the converted gray images
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(_ap())))
        rc, bufs = _ctx_run(ctx, gray, fields, (rgb_l, rgb_r), 3, PDMINL)
        _lib.check(rc)
        for k, v in bufs.items():
            _eq(v, gray[NAMES[k]], f"gray AD through the rgb entry {k}")
        # colour 1 with the gray guide: the pipeline's (= the oracle's) maps; three and four channels
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(_ap(colour=1))))
        rgba = [np.concatenate((x, np.full((PH, PW, 1), 9, np.uint8)), axis=2) for x in (rgb_l, rgb_r)]
        for imgs, ch in (((rgb_l, rgb_r), 3), (rgba, 4)):
            for f in ([k for k in fields if not k.startswith(("cost", "agg"))], fields):
                rc, bufs = _ctx_run(ctx, e, f, imgs, ch, PDMINL)
                _lib.check(rc)
                for k, v in bufs.items():
                    _eq(v, e[NAMES[k]], f"colour AD, {ch} channels, {k}")
        rc, _ = _ctx_run(ctx, e, ["filled"], (s["Il"], s["Ir"]), 0, PDMINL)
        assert rc == -1 and b"smx_ctx_stereo_pair_rgb" in L.smx_last_error()
        # with the colour guide: the colour-guided pipeline's maps
        _lib.check(L.smx_ctx_set_guidance(ctx, 1))
        c = _finish(orc, dict({k: colour_chain[k] for k in ("aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr")}, costl=s["costl"],
                              costr=s["costr"]), PDMINL)
        for f in (["best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled"], fields):
            rc, bufs = _ctx_run(ctx, c, f, (rgb_l, rgb_r), 3, PDMINL)
            _lib.check(rc)
            for k, v in bufs.items():
                _eq(v, c[NAMES[k]], f"colour AD and colour guide {k}")
    finally:
        L.smx_destroy(ctx)


# ---------------------------------------------------------------------------------------------
# graph capture; the default
# ---------------------------------------------------------------------------------------------
def test_pair_step_is_capturable_in_a_hip_graph(orc):
    """Eager, capture, two replays after zeroing the buffers.  The table was uploaded by the constructor: outside the capture."""
    import torch
    w, h, D = PAIRS["129x70"]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    pipe = _pipe(Il, Ir, D, run=False, slices_in_flight=32)
    imgs = _t(np.stack([Il, Ir]))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pipe.run(imgs[0], imgs[1])               # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = pipe.results()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pipe.run(imgs[0], imgs[1])
    pipe.keys.zero_()
    pipe.codes.zero_()
    pipe.census_cost.zero_()
    pipe.filled.zero_()
    for _ in range(2):
        g.replay()
    r = pipe.results()
    for k in MAPS:
        _eq(r[k], eager[k], "graph against eager " + k)
        _eq(r[k], e[k], "graph " + k)


def test_the_default_cost_is_unchanged(orc):
    from stereo_matching_cuda_amd.device import PairPipeline
    w, h, D = PAIRS["129x70"]
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    want = orc.stereo_pair(Il, Ir, D)
    pipe = PairPipeline(w, h, D)
    assert pipe.cost is None and pipe.codes is None and pipe.census_cost is None and pipe.census_params is None
    assert pipe.adcensus_params is None and pipe.adcensus_table is None
    pipe.run(_t(Il), _t(Ir))
    r = pipe.results()
    for k in MAPS:
        _eq(r[k], want[k], k)
    assert np.any(want["dmapl"] != expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")["dmapl"])
    census = PairPipeline(w, h, D, cost="census")
    assert census.adcensus_params is None and census.adcensus_table is None
