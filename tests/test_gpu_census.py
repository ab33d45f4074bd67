"""The census / Hamming matching cost on the GPU (smx_dev_census, smx_dev_census_cost_pair, smx_census_cost,
PairPipeline(cost="census"), smx_ctx_set_cost and smx_main --cost census).  The two kernels are held to tests/census_ref.py
bit for bit; everything behind them to the oracle fed with the reference's volume: oracle.guided_filter for both views ->
oracle.detect_occlusion -> oracle.fill_occlusion.  All comparisons are equality.

k_census works on 64 x 8 tiles, k_census_cost_pair on 256 columns x 16 slices: the shapes aim at those edges.

Run on the GPU box:  python -m pytest tests -m gpu -q -k census
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import census_ref as ref
from main_harness import main_cases  # noqa: F401  (a fixture)
import subpix_ref
import wmf_ref

pytestmark = pytest.mark.gpu

WINDOWS = [(1, 1), (4, 1), (2, 3), (4, 3)]
MAPS = ("bestl", "bestr", "dmapl", "dmapr", "meanl", "meanr", "occlusion", "filled")


def _eq(a, b, name=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _cp(rx=4, ry=3, th=62):
    p = _lib.CensusParams()
    p.rx, p.ry, p.th = rx, ry, th
    return p


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _codes(Il, Ir, p):
    """The codes of a pair, one launch for both images -> device tensor (2, h, w) int64."""
    import torch
    imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
    h, w = Il.shape
    codes = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    _lib.check(smx.lib().smx_dev_census(C.byref(p), _dp(imgs), _dp(codes), w, h, 2, _stream()))
    return codes


def _cost_pair(codes, p, dminl, dminr, s0, s1, left=True, right=True):
    """smx_dev_census_cost_pair -> (left volume or None, right volume or None) as numpy, each with a guard plane behind
    it that must stay untouched."""
    import torch
    _, h, w = codes.shape
    out = [torch.full((s1 - s0 + 1, h, w), -7.0, device="cuda") if on else None for on in (left, right)]
    _lib.check(smx.lib().smx_dev_census_cost_pair(C.byref(p), _dp(codes), _dp(out[0]), _dp(out[1]), w, h, dminl, dminr,
                                                  s0, s1, _stream()))
    res = []
    for t in out:
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert np.all(a[-1] == -7.0), "the launch wrote behind its slices"
        res.append(a[:-1])
    return res


def _rand_pair(w, h, seed, hi=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, hi, size=(h, w), dtype=np.uint8), rng.integers(0, hi, size=(h, w), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------
def _transform_images():
    rng = np.random.default_rng(5)
    imgs = {f"{w}x{h}": rng.integers(0, 256, size=(h, w), dtype=np.uint8) for w, h in ((3, 2), (1, 1), (64, 8), (65, 9), (129, 70))}
    # few gray levels: equal neighbours everywhere
    imgs["129x70 coarse"] = (rng.integers(0, 4, size=(70, 129)) * 60).astype(np.uint8)
    imgs["constant"] = np.full((20, 70), 131, np.uint8)
    two = np.where(rng.random((20, 70)) < 0.5, 40, 41).astype(np.uint8)
    imgs["two values"] = two
    return imgs


@pytest.mark.parametrize("rx,ry", WINDOWS)
def test_transform(rx, ry):
    for name, img in _transform_images().items():
        got = smx.census_transform(img, _cp(rx, ry))
        want = ref.census_transform(img, rx, ry)
        _eq(got, want, f"{name} window {rx},{ry}")
        assert int(got.max()) < 1 << ref.nbits(rx, ry)
        if name == "constant":
            assert not got.any()
        if name == "two values":
            assert got.any() and not got[img == 40].any()          # `<`, not `<=`


def test_transform_of_a_pair_in_one_launch():
    Il, Ir = _rand_pair(131, 19, 3)
    codes = _codes(Il, Ir, _cp()).cpu().numpy().view(np.uint64)
    _eq(codes[0], ref.census_transform(Il), "left")
    _eq(codes[1], ref.census_transform(Ir), "right")


# ---------------------------------------------------------------------------------------------
# the cost
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dmin,D", [(-69, 70), (-5, 12), (3, 4), (-2, 1), (-200, 3), (150, 2)])
def test_cost_ranges(dmin, D):
    """Labels left of zero, right of it, across it, one slice, and ranges that lie outside the image altogether."""
    Il, Ir = _rand_pair(97, 5, D)
    p = _cp()
    dminr = -(dmin + D - 1)
    codes = _codes(Il, Ir, p)
    cl, cr = _cost_pair(codes, p, dmin, dminr, 0, D)
    _eq(cl, ref.census_cost(Il, Ir, D, dmin), "left")
    _eq(cr, ref.census_cost(Ir, Il, D, dminr), "right")
    if abs(dmin) >= 150:
        assert np.all(cl == 62.0)


@pytest.mark.parametrize("s0,s1", [(0, 1), (3, 20), (16, 49), (15, 17), (69, 70), (5, 5)])
def test_cost_slice_ranges(s0, s1):
    """Sub-ranges whose length is no multiple of the 16 slices of a workgroup; an empty one launches nothing."""
    Il, Ir = _rand_pair(70, 4, 9)
    p = _cp(2, 3, 20)
    codes = _codes(Il, Ir, p)
    cl, cr = _cost_pair(codes, p, -69, 0, s0, s1)
    _eq(cl, ref.census_cost(Il, Ir, 70, -69, 2, 3, 20, s0, s1), "left")
    _eq(cr, ref.census_cost(Ir, Il, 70, 0, 2, 3, 20, s0, s1), "right")


@pytest.mark.parametrize("w", [255, 256, 257])
def test_cost_at_the_column_edges_of_a_workgroup(w):
    Il, Ir = _rand_pair(w, 3, w)
    p = _cp(4, 1, 30)
    codes = _codes(Il, Ir, p)
    cl, cr = _cost_pair(codes, p, -5, -6, 0, 12)
    _eq(cl, ref.census_cost(Il, Ir, 12, -5, 4, 1, 30), "left")
    _eq(cr, ref.census_cost(Ir, Il, 12, -6, 4, 1, 30), "right")


@pytest.mark.parametrize("rx,ry", [(1, 1), (4, 3)])
def test_cost_truncation(rx, ry):
    Il, Ir = _rand_pair(67, 9, rx)
    nb = ref.nbits(rx, ry)
    for th in (1, 5, nb, nb + 10):
        p = _cp(rx, ry, th)
        cl, cr = _cost_pair(_codes(Il, Ir, p), p, -4, -1, 0, 6)
        _eq(cl, ref.census_cost(Il, Ir, 6, -4, rx, ry, th), f"left th {th}")
        _eq(cr, ref.census_cost(Ir, Il, 6, -1, rx, ry, th), f"right th {th}")
        assert cl.max() == min(th, nb)


def test_single_view_forms_and_the_host_entry():
    Il, Ir = _rand_pair(131, 7, 1)
    p = _cp(4, 3, 40)
    codes = _codes(Il, Ir, p)
    both = _cost_pair(codes, p, -17, 2, 0, 19)
    left, none = _cost_pair(codes, p, -17, 2, 0, 19, right=False)
    none2, right = _cost_pair(codes, p, -17, 2, 0, 19, left=False)
    assert none is None and none2 is None
    _eq(left, both[0], "left alone")
    _eq(right, both[1], "right alone")
    _eq(smx.census_cost(Il, Ir, 19, -17, p), both[0], "host entry, left")
    _eq(smx.census_cost(Ir, Il, 19, 2, p), both[1], "host entry, right")
    _eq(both[0], ref.census_cost(Il, Ir, 19, -17, 4, 3, 40), "reference")


def test_invariance_under_an_increasing_map_of_one_image():
    """What the feature is for: R -> 2 R + 1 (another gain and offset) leaves the census volumes untouched, bit for bit, and
    changes the reference's cost."""
    Il, Ir = synth.gen_pair(150, 40, 16, 12)
    Il, Ir = (Il // 2).astype(np.uint8), (Ir // 2).astype(np.uint8)
    Ir2 = (2 * Ir + 1).astype(np.uint8)
    p = _cp()
    a = _cost_pair(_codes(Il, Ir, p), p, -15, 0, 0, 16)
    b = _cost_pair(_codes(Il, Ir2, p), p, -15, 0, 0, 16)
    _eq(b[0], a[0], "left")
    _eq(b[1], a[1], "right")
    assert len(np.unique(a[0])) > 10
    assert not np.array_equal(smx.compute_cost(Il, Ir2, 16, -15), smx.compute_cost(Il, Ir, 16, -15))


# ---------------------------------------------------------------------------------------------
# end to end: the pipeline against the oracle fed with the reference's volumes
# ---------------------------------------------------------------------------------------------
_EXPECTED = {}


def expected(orc, Il, Ir, D, dminl, dminr, radius=9, cp=(4, 3, 62), tag=None):
    """The maps of a pair: census_ref cost -> oracle.guided_filter for both views -> detect_occlusion -> fill_occlusion."""
    key = (tag, D, dminl, dminr, radius, cp)
    if tag is None or key not in _EXPECTED:
        P = orc.Params()
        smxp = smx.default_params()
        for f, _ in orc.Params._fields_:
            setattr(P, f, getattr(smxp, f))
        P.radius = radius
        cl = ref.census_cost(Il, Ir, D, dminl, *cp)
        cr = ref.census_cost(Ir, Il, D, dminr, *cp)
        bl, ml, meanl, aggl = orc.guided_filter(Il, cl, dminl, want_agg=True, params=P)
        br, mr, meanr, aggr = orc.guided_filter(Ir, cr, dminr, want_agg=True, params=P)
        occ = orc.detect_occlusion(ml, mr, dminl - 100, params=P)
        e = dict(costl=cl, costr=cr, bestl=bl, bestr=br, dmapl=ml, dmapr=mr, meanl=meanl, meanr=meanr, aggl=aggl, aggr=aggr,
                 occlusion=occ, filled=orc.fill_occlusion(occ, float(dminl)))
        if tag is None:
            return e
        _EXPECTED[key] = e
    return _EXPECTED[key]


def _pipe(Il, Ir, D, radius=9, census_params=None, run=True, **kw):
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    p = smx.default_params()
    p.radius = radius
    pipe = PairPipeline(w, h, D, params=p, cost="census", census_params=census_params, **kw)
    if run:
        imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
        pipe.run(imgs[0], imgs[1])
    return pipe


PAIRS = {"129x70": (129, 70, 70), "210x150": (210, 150, 32)}


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
    if radius == 9:                                 # small non-negative integers: the comb walker's check never fires
        rr = C.c_int(-1)
        _lib.check(smx.lib().smx_dev_agg_fallback(_dp(pipe.ws), C.byref(rr)))
        assert rr.value == 0


def test_chunks_and_split_calls(orc):
    import torch
    w, h, D = 97, 40, 19
    Il, Ir = synth.gen_pair(w, h, D, 8)
    e = expected(orc, Il, Ir, D, -(D - 1), 0)
    keys = None
    for sif in (1, 7, D):
        pipe = _pipe(Il, Ir, D, slices_in_flight=sif, want_agg=True)
        assert pipe.slices_in_flight == sif and pipe.census_cost.shape == (2, sif, h, w)
        r = pipe.results()
        for k in MAPS + ("aggl", "aggr"):
            _eq(r[k], e[k], f"slices_in_flight {sif} {k}")
        k64 = pipe.keys.cpu().numpy()
        if keys is not None:
            _eq(k64, keys, f"keys, slices_in_flight {sif}")
        keys = k64
    # a byte bound halves the slices in flight, the census buffer counted
    fits = 2 * smx.lib().smx_agg_workspace_bytes_for(C.byref(smx.default_params()), w, h, D) + 2 * D * w * h * 4
    assert _pipe(Il, Ir, D, run=False, max_ws_bytes=fits).slices_in_flight == D
    assert _pipe(Il, Ir, D, run=False, max_ws_bytes=fits - 1).slices_in_flight == (D + 1) // 2
    # two calls over [0, k) and [k, D) on the device entries accumulate to the same keys
    L = smx.lib()
    p = _cp()
    codes = _codes(Il, Ir, p)
    imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
    for k in (1, 7, D - 1):
        pipe = _pipe(Il, Ir, D, run=False)
        pipe.keys.fill_(0)
        cost = torch.empty((2, D, h, w), device="cuda")
        for s0, s1, fresh in ((0, k, 1), (k, D, 0)):
            _lib.check(L.smx_dev_census_cost_pair(C.byref(p), _dp(codes), _dp(cost[0]), _dp(cost[1]), w, h, pipe.dminl,
                                                  pipe.dminr, s0, s1, _stream()))
            L.smx_set_keys_fresh(fresh)
            try:
                _lib.check(L.smx_dev_aggregate_wta_pair_cost(
                    C.byref(pipe.params), _dp(imgs[0]), _dp(imgs[1]), _dp(cost[0]), _dp(cost[1]), w, h, pipe.dminl,
                    pipe.dminr, s0, s1, _dp(pipe.keys), _dp(pipe.mean), None, _dp(pipe.ws), pipe.ws_bytes, _stream()))
            finally:
                L.smx_set_keys_fresh(0)
        pipe.finish()
        _eq(pipe.keys.cpu().numpy(), keys, f"keys, split at {k}")
        _eq(pipe.results()["filled"], e["filled"], f"filled, split at {k}")
    # a pipeline over a sub-range of the slices: the oracle over that range
    P = orc.Params()
    for f, _ in orc.Params._fields_:
        setattr(P, f, getattr(smx.default_params(), f))
    sub = _pipe(Il, Ir, D, s_begin=3, s_end=14, slices_in_flight=4, want_agg=True).results()
    for v, (img, c) in enumerate(((Il, e["costl"]), (Ir, e["costr"]))):
        best, dmap, _, agg = orc.guided_filter(img, c, (-(D - 1), 0)[v], s_begin=3, s_end=14, want_agg=True, params=P)
        _eq(sub["best" + "lr"[v]], best, "sub-range best")
        _eq(sub["dmap" + "lr"[v]], dmap, "sub-range dmap")
        _eq(sub["agg" + "lr"[v]], agg, "sub-range agg")


def test_composition_with_subpixel_and_weighted_median(orc):
    w, h, D = 129, 70, 70
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    pipe = _pipe(Il, Ir, D, subpixel="parabola", wmf="all", slices_in_flight=16)
    r = pipe.results()
    for k in MAPS:
        _eq(r[k], e[k], k)
    subs = []
    for v, (agg, dmap) in enumerate(((e["aggl"], e["dmapl"]), (e["aggr"], e["dmapr"]))):
        z, c0, lo, hi, _ = subpix_ref.winners(agg)
        subs.append(subpix_ref.maps(subpix_ref.PARABOLA, z, c0, lo, hi, dmap, e["occlusion"] if v == 0 else None,
                                    e["filled"], -(D - 1)))
    _eq(r["subpixl"], subs[0][0], "subpixl")
    _eq(r["subpixr"], subs[1][0], "subpixr")
    _eq(r["subpix_filled"], subs[0][1], "subpix_filled")
    assert np.any(subs[0][0] != e["dmapl"])
    want = wmf_ref.weighted_median(Il, e["filled"], -(D - 1), D, None)
    _eq(r["refined"], want, "refined")
    assert np.any(want != e["filled"])


def test_context(orc):
    w, h, D = 129, 70, 70
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    plain = orc.stereo_pair(Il, Ir, D, want_cost=True)
    L = smx.lib()
    n = w * h
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), w, h, D, C.byref(ctx)))
    try:
        names = {"best_l": "bestl", "best_r": "bestr", "dmap_l": "dmapl", "dmap_r": "dmapr", "occlusion": "occlusion",
                 "filled": "filled", "mean_l": "meanl", "mean_r": "meanr", "cost_l": "costl", "cost_r": "costr",
                 "agg_l": "aggl", "agg_r": "aggr"}

        def run(fields):
            bufs = {k: np.empty(e[names[k]].shape, e[names[k]].dtype) for k in fields}
            out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
            _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, -(D - 1), 0, C.byref(out)))
            return bufs

        assert L.smx_ctx_set_cost(ctx, 2, None) == -1 and L.smx_ctx_set_cost(ctx, -1, None) == -1
        bad = _cp(5, 3, 62)
        assert L.smx_ctx_set_cost(ctx, 1, C.byref(bad)) == -1
        maps = [k for k in names if not k.startswith(("cost", "agg"))]
        _lib.check(L.smx_ctx_set_cost(ctx, _lib.COST_MODES["census"], None))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -(D - 1), 0) == -1
        for fields in (maps, list(names)):                      # through the chunk buffer, then with the whole volumes
            for k, v in run(fields).items():
                _eq(v, e[names[k]], f"census ctx {k}")
        # other parameters
        e2 = expected(orc, Il, Ir, D, -(D - 1), 0, 9, cp=(2, 1, 9))
        p2 = _cp(2, 1, 9)
        _lib.check(L.smx_ctx_set_cost(ctx, 1, C.byref(p2)))
        for k, v in run(maps).items():
            _eq(v, e2[names[k]], f"census 5x3 ctx {k}")
        # and back
        _lib.check(L.smx_ctx_set_cost(ctx, _lib.COST_MODES["reference"], None))
        for k, v in run(maps + ["cost_l", "cost_r"]).items():
            _eq(v, plain[names[k]], f"reference ctx {k}")
        _lib.check(L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -(D - 1), 0))
        _lib.check(L.smx_ctx_wait(ctx, None, None))
    finally:
        L.smx_destroy(ctx)


def test_context_chunks_do_not_change_a_bit(orc):
    """The context's chunk loop of the guided flow from census codes under smx_set_max_slices_per_launch: at 16 slices, 5 gives
    chunks of 5, 5, 5 and a ragged last one of a single slice, 16 one chunk, 1 every slice alone; every chunk after the first
    accumulates into the keys.  Through the chunk buffer, then with the whole volumes, where the aggregated slices go to
    their offsets.  Against the reference chain of test_context."""
    w, h, D, dminl = 129, 70, 16, -15
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, dminl, 0, 9, tag="129x70x16")
    L = smx.lib()
    names = {"best_l": "bestl", "best_r": "bestr", "dmap_l": "dmapl", "dmap_r": "dmapr", "occlusion": "occlusion",
             "filled": "filled", "mean_l": "meanl", "mean_r": "meanr", "cost_l": "costl", "cost_r": "costr",
             "agg_l": "aggl", "agg_r": "aggr"}
    maps = [k for k in names if not k.startswith(("cost", "agg"))]
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), w, h, D, C.byref(ctx)))
    try:
        _lib.check(L.smx_ctx_set_cost(ctx, _lib.COST_MODES["census"], None))
        for k in (1, 5, 16):
            for fields in (maps, list(names)):
                bufs = {f: np.empty(e[names[f]].shape, e[names[f]].dtype) for f in fields}
                out = _lib.PairOut(**{f: v.ctypes.data for f, v in bufs.items()})
                _lib.check(L.smx_set_max_slices_per_launch(k))
                try:
                    rc = L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0, C.byref(out))
                finally:
                    L.smx_set_max_slices_per_launch(0)
                _lib.check(rc)
                for f, v in bufs.items():
                    _eq(v, e[names[f]], f"census ctx, at most {k} slices, {len(fields)} planes: {f}")
    finally:
        L.smx_destroy(ctx)
    assert len(np.unique(e["dmapl"])) > 3


def test_pair_step_is_capturable_in_a_hip_graph(orc):
    import torch
    w, h, D = 129, 70, 70
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    e = expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")
    pipe = _pipe(Il, Ir, D, run=False, slices_in_flight=32)
    imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
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
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    w, h, D = 129, 70, 70
    Il, Ir = synth.gen_pair(w, h, D, w + h)
    want = orc.stereo_pair(Il, Ir, D)
    pipe = PairPipeline(w, h, D)
    assert pipe.cost is None and pipe.codes is None and pipe.census_cost is None and pipe.census_params is None
    pipe.run(torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda())
    r = pipe.results()
    for k in MAPS:
        _eq(r[k], want[k], k)
    assert np.any(want["dmapl"] != expected(orc, Il, Ir, D, -(D - 1), 0, 9, tag="129x70")["dmapl"])


# ---------------------------------------------------------------------------------------------
# smx_main --cost census
# ---------------------------------------------------------------------------------------------
def _rgb_pair(orc):
    w, h, D = 129, 70, 24
    gl, gr = synth.gen_pair(w, h, D, 77)
    rng = np.random.default_rng(2)
    left, right = (np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8) for g in (gl, gr))
    left[..., 1] += rng.integers(0, 3, size=(h, w), dtype=np.uint8)
    return left, right, orc.gray(left), orc.gray(right), D


@pytest.mark.parametrize("flags,cp", [(["--cost", "census"], (4, 3, 62)),
                                      (["--cost", "census", "--census-window", "5x3", "--census-th", "9"], (2, 1, 9))],
                         ids=["defaults", "5x3_th9"])
def test_main_writes_the_census_maps(orc, main_cases, tmp_path, flags, cp):
    mc = main_cases
    left, right, gl, gr, D = _rgb_pair(orc)
    e = dict(expected(orc, gl, gr, D, -(D - 1), 0, 9, cp=cp))
    e.update(grayl=gl, grayr=gr, cost0l=e["costl"][0].copy(), cost0r=e["costr"][0].copy())
    r, files = mc.run_main(mc.BIN, tmp_path, left, right, [-(D - 1), 0], flags, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    mc.check_twelve(orc, files, e, " ".join(flags))
    mc.check_disparity_files(files, e["filled"], 129, 70, " ".join(flags))


@pytest.mark.parametrize("flags", [["--cost", "census", "--ngpu", "1"],
                                   ["--cost", "census", "--fused", "--pairs", "3", "--pipeline"],
                                   ["--cost", "census", "--census-window", "4x3"],
                                   ["--cost", "census", "--census-window", "11x7"],
                                   ["--cost", "census", "--census-th", "0"],
                                   ["--cost", "hamming"]],
                         ids=["ngpu", "pipeline", "even_window", "wide_window", "th0", "unknown_cost"])
def test_main_refuses(orc, main_cases, tmp_path, flags):
    mc = main_cases
    left, right, _, _, D = _rgb_pair(orc)
    r, files = mc.run_main(mc.BIN, tmp_path, left, right, [-(D - 1), 0], flags, timeout=60)
    assert r.returncode == 2 and ("--cost" in r.stderr or "--census" in r.stderr), (r.returncode, r.stdout + r.stderr)
    assert not files["png"]
