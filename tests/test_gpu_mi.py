"""The mutual-information matching cost on the GPU (csrc/smx_mi.hip), bit for bit against tests/mi_ref.py:
  smx_dev_mi_histogram   random images and maps with a third of the pixels marked, labels that send partners off both edges, a
                         flat pair whose pixels all meet in one counter (more than 65 535 of them), a map that is invalid
                         everywhere, two calls in a row on one buffer
  smx_dev_mi_cost_pair   size_d 1 / 16 / 70, dmin negative, zero and positive, sub-ranges of the slices, each view alone, an
                         asymmetric table (a swapped index in the right view shows) and a table of one cheap cell
  behind the cost        the MI volumes through the comb walker (no fall-back), the multi-kernel path and SGM against the oracle
                         and sgm_ref fed with the numpy volume
  context, PairPipeline  the loop of smx_ctx_set_mi against mi_ref.pair_loop on the scene of DESIGN.md 4.3s

k_mi_cost_pair works on 256 columns x 4 rows and stages the partner pixels of 256 slices at a time; the histogram takes 256
pixels a workgroup: the shapes aim at those edges.

Run on the GPU box:  python -m pytest tests -m gpu -q -k mi
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import mi_ref as ref
import perm_ref
import sgm_ref
import subpix_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
PRESET = np.uint32(0x7F7F7F7F).view(F32)
SHAPES = [(1, 1), (2, 1), (64, 9), (129, 70), (210, 150)]          # (w, h)
MAPS = ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled")


def _eq(a, b, name=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rand_pair(w, h, seed, hi=256):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, hi, size=(h, w), dtype=np.uint8), rng.integers(0, hi, size=(h, w), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------
# the histogram
# ---------------------------------------------------------------------------------------------
def _dev_histogram(Il, Ir, disp, mark, hist=None):
    import torch
    h, w = Il.shape
    if hist is None:
        hist = torch.full((257, 256), 7, dtype=torch.int32, device="cuda")      # (a guard row behind the counters)
    il, ir, m = _t(Il), _t(Ir), _t(disp)          # (named: a temporary would be freed, and its memory reused, before the launch)
    _lib.check(smx.lib().smx_dev_mi_histogram(_dp(il), _dp(ir), _dp(m), float(mark), _dp(hist), w, h, _stream()))
    a = hist.cpu().numpy().view(np.uint32)
    assert np.all(a[256] == 7), "the launch wrote behind the counters"
    return a[:256], hist


@pytest.mark.parametrize("w,h", SHAPES)
def test_histogram(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    Il, Ir = _rand_pair(w, h, w + h)
    mark = F32(-115)
    # labels -w - 2 .. w + 2: partners off both edges; about a third of the pixels carry the mark
    disp = rng.integers(-w - 2, w + 3, size=(h, w)).astype(F32)
    disp[rng.random((h, w)) < 1 / 3] = mark
    got, hist = _dev_histogram(Il, Ir, disp, mark)
    want = ref.histogram(Il, Ir, disp, mark)
    _eq(got, want, f"{w}x{h}")
    assert want.sum() < w * h or w * h == 1
    _eq(smx.mi_histogram(Il, Ir, disp, mark), want, f"{w}x{h} host entry")
    # a second call on the same buffer starts from zero again
    disp2 = np.zeros((h, w), F32)
    got2, _ = _dev_histogram(Il, Ir, disp2, mark, hist)
    _eq(got2, ref.histogram(Il, Ir, disp2, mark), f"{w}x{h} second call")
    assert got2.sum() == w * h
    # a map that is invalid everywhere
    got3, _ = _dev_histogram(Il, Ir, np.full((h, w), mark, F32), mark, hist)
    assert not got3.any()


def test_histogram_of_a_flat_pair_meets_in_one_counter():
    w = h = 300
    Il, Ir = np.full((h, w), 131, np.uint8), np.full((h, w), 77, np.uint8)
    disp = np.full((h, w), -3, F32)
    got, _ = _dev_histogram(Il, Ir, disp, -115)
    _eq(got, ref.histogram(Il, Ir, disp, -115), "flat")
    assert got[131, 77] == h * (w - 3) and got[131, 77] > 65535 and got.sum() == got[131, 77]


# ---------------------------------------------------------------------------------------------
# the cost
# ---------------------------------------------------------------------------------------------
def _tables():
    rng = np.random.default_rng(11)
    asym = rng.integers(0, 256, size=(256, 256), dtype=np.uint8)
    assert not np.array_equal(asym, asym.T)
    cell = np.full((256, 256), 255, np.uint8)
    cell[40, 200] = 3
    return {"asymmetric": asym, "one cell": cell}


def _cost_pair(T, Il, Ir, dminl, dminr, s0, s1, left=True, right=True):
    """smx_dev_mi_cost_pair -> (left volume or None, right volume or None), each with a guard plane behind it."""
    import torch
    h, w = Il.shape
    out = [torch.full((s1 - s0 + 1, h, w), -7.0, device="cuda") if on else None for on in (left, right)]
    tab, il, ir = _t(T), _t(Il), _t(Ir)           # (named: a temporary would be freed, and its memory reused, before the launch)
    _lib.check(smx.lib().smx_dev_mi_cost_pair(_dp(tab), _dp(il), _dp(ir), _dp(out[0]), _dp(out[1]), w, h, dminl, dminr,
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


@pytest.mark.parametrize("D", [1, 16, 70])
@pytest.mark.parametrize("w,h", SHAPES)
def test_cost(w, h, D):
    Il, Ir = _rand_pair(w, h, w + h + D)
    if w >= 64:                              # the one cheap cell of the second table occurs
        Il[:, ::7], Ir[:, 3::7] = 40, 200
    for name, T in _tables().items():
        for dminl, dminr in ((-(D - 1), 0), (0, -(D - 1)), (2, -D - 1)):
            cl, cr = _cost_pair(T, Il, Ir, dminl, dminr, 0, D)
            _eq(cl, ref.cost(T, Il, Ir, D, dminl), f"{name} left {dminl}")
            _eq(cr, ref.cost(T, Il, Ir, D, dminr, right=True), f"{name} right {dminr}")
    if w >= 64 and D > 1:
        assert (cl == 3.0).any() or (cr == 3.0).any()
        assert cl.max() == 255.0


@pytest.mark.parametrize("s0,s1", [(0, 1), (3, 20), (16, 49), (69, 70), (5, 5)])
def test_cost_slice_ranges(s0, s1):
    Il, Ir = _rand_pair(129, 9, 9)
    T = _tables()["asymmetric"]
    cl, cr = _cost_pair(T, Il, Ir, -69, 0, s0, s1)
    _eq(cl, ref.cost(T, Il, Ir, 70, -69, s_begin=s0, s_end=s1), "left")
    _eq(cr, ref.cost(T, Il, Ir, 70, 0, True, s0, s1), "right")


def test_two_adjoining_ranges_equal_the_whole_and_single_view_forms():
    Il, Ir = _rand_pair(210, 11, 1)
    T = _tables()["asymmetric"]
    D, dl, dr = 70, -40, -29
    whole = _cost_pair(T, Il, Ir, dl, dr, 0, D)
    a, b = _cost_pair(T, Il, Ir, dl, dr, 0, 23), _cost_pair(T, Il, Ir, dl, dr, 23, D)
    for v, side in enumerate(("left", "right")):
        _eq(np.concatenate([a[v], b[v]]), whole[v], f"{side}: [0, 23) + [23, 70)")
    left, none = _cost_pair(T, Il, Ir, dl, dr, 0, D, right=False)
    none2, right = _cost_pair(T, Il, Ir, dl, dr, 0, D, left=False)
    assert none is None and none2 is None
    _eq(left, whole[0], "left alone")
    _eq(right, whole[1], "right alone")
    _eq(smx.mi_cost(T, Il, Ir, D, dl), whole[0], "host entry, left")
    _eq(smx.mi_cost(T, Ir, Il, D, dr, right=True), whole[1], "host entry, right")
    tab, il, ir = _t(T), _t(Il), _t(Ir)
    assert smx.lib().smx_dev_mi_cost_pair(_dp(tab), _dp(il), _dp(ir), None, None, 210, 11, dl, dr, 0, D, _stream()) == -1


@pytest.mark.parametrize("w", [255, 256, 257])
def test_cost_at_the_column_edges_of_a_workgroup(w):
    Il, Ir = _rand_pair(w, 5, w)
    T = _tables()["asymmetric"]
    cl, cr = _cost_pair(T, Il, Ir, -5, -6, 0, 12)
    _eq(cl, ref.cost(T, Il, Ir, 12, -5), "left")
    _eq(cr, ref.cost(T, Il, Ir, 12, -6, True), "right")


def test_cost_over_more_slices_than_one_staged_span():
    Il, Ir = _rand_pair(300, 3, 5)
    T = _tables()["asymmetric"]
    cl, cr = _cost_pair(T, Il, Ir, -299, 0, 0, 300)
    _eq(cl, ref.cost(T, Il, Ir, 300, -299), "left")
    _eq(cr, ref.cost(T, Il, Ir, 300, 0, True), "right")


def test_random_map():
    import torch
    for (w, h), D, dmin, seed in zip(SHAPES, (1, 3, 16, 70, 192), (0, -2, -15, 5, -191), (0, 1, 2, 0xFFFFFFFF, 7)):
        m = torch.full((h + 1, w), -7.0, device="cuda")
        _lib.check(smx.lib().smx_dev_mi_random_map(_dp(m), w, h, dmin, D, seed, _stream()))
        a = m.cpu().numpy()
        assert np.all(a[h] == -7.0)
        _eq(a[:h], ref.random_map(w, h, dmin, D, seed), f"{w}x{h}")


# ---------------------------------------------------------------------------------------------
# behind the cost: 129 x 70 x 16
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL, DMINR = 129, 70, 16, -15, 0


@pytest.fixture(scope="module")
def volumes():
    """A pair, the table its true-ish labels give, and the numpy volumes of both views."""
    Il, Ir = synth.gen_pair(W, H, D, W + H)
    Ir = (255 - Ir).astype(np.uint8)
    T = ref.table(ref.histogram(Il, Ir, np.full((H, W), -4, F32), DMINL - 100))
    return Il, Ir, T, ref.cost(T, Il, Ir, D, DMINL), ref.cost(T, Il, Ir, D, DMINR, right=True)


def _pipe(Il, Ir, T, **kw):
    """One pass of a cost="mi" pipeline with the table T: aggregate() and the finish, no loop."""
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(W, H, D, dminl=DMINL, dminr=DMINR, cost="mi", **kw)
    pipe.mi_table.copy_(_t(T))
    pipe.aggregate(_t(Il), _t(Ir))
    pipe.finish()
    return pipe


@pytest.mark.parametrize("radius,path", [(9, 5), (12, 1)])
def test_guided_filter_from_the_mi_volumes(orc, volumes, radius, path):
    Il, Ir, T, cl, cr = volumes
    P = orc.Params()
    for f, _ in orc.Params._fields_:
        setattr(P, f, getattr(smx.default_params(), f))
    P.radius = radius
    p = smx.default_params()
    p.radius = radius
    pipe = _pipe(Il, Ir, T, params=p, want_agg=True)
    assert smx.lib().smx_last_agg_path() == path
    got = pipe.results()
    bl, ml, _, al = orc.guided_filter(Il, cl, DMINL, want_agg=True, params=P)
    br, mr, _, ar = orc.guided_filter(Ir, cr, DMINR, want_agg=True, params=P)
    for k, want in (("bestl", bl), ("bestr", br), ("dmapl", ml), ("dmapr", mr), ("aggl", al), ("aggr", ar)):
        _eq(got[k], want, f"radius {radius} {k}")
    _eq(pipe.keys.cpu().numpy(), np.stack([orc.pack_keys(bl, (ml - DMINL).astype(np.int64)),
                                          orc.pack_keys(br, (mr - DMINR).astype(np.int64))]), "keys")
    assert len(np.unique(ml)) > 3
    if path == 5:                               # integers 0 .. 255: the comb walker's check never fires
        rr = C.c_int(-1)
        _lib.check(smx.lib().smx_dev_agg_fallback(_dp(pipe.ws), C.byref(rr)))
        assert rr.value == 0


def test_sgm_from_the_mi_volumes(volumes):
    Il, Ir, T, cl, cr = volumes
    pipe = _pipe(Il, Ir, T, aggregation="sgm", want_agg=True)
    got = pipe.results()
    sl, sr = sgm_ref.outputs(cl), sgm_ref.outputs(cr)
    _eq(pipe.keys.cpu().numpy(), np.stack([sl["keys"], sr["keys"]]), "keys")
    _eq(got["aggl"], sl["agg"], "aggl")
    _eq(got["aggr"], sr["agg"], "aggr")
    _eq(got["dmapl"], (DMINL + sl["z"]).astype(F32), "dmapl")


# ---------------------------------------------------------------------------------------------
# the loop: context and pipeline on the scene
# ---------------------------------------------------------------------------------------------
SW, SH, SD, SDMINL, SDMINR = ref.SCENE_W, ref.SCENE_H, ref.SCENE_D, ref.SCENE_DMIN, 0
SIGMA = 32.0
SETTINGS = ("guided", "sgm", "permeability")


def _solver(orc, Il, Ir, setting):
    def guided(I, c, dmin):
        return orc.guided_filter(I, c, dmin, want_agg=True)

    def solve(cl, cr):
        r = {}
        for side, I, c, dmin in (("l", Il, cl, SDMINL), ("r", Ir, cr, SDMINR)):
            if setting == "sgm":
                s = sgm_ref.outputs(c)
                r["best" + side], r["dmap" + side] = s["best"], (dmin + s["z"]).astype(F32)
            elif setting == "permeability":
                z, c0 = subpix_ref.winners(perm_ref.filter_volume(guided(I, c, dmin)[3], I, SIGMA))[:2]
                r["dmap" + side] = subpix_ref.dmap_of(z, c0, dmin)
                r["best" + side] = np.where((z >= 0) & (PRESET >= c0), c0, PRESET).astype(F32)
            else:
                r["best" + side], r["dmap" + side] = guided(I, c, dmin)[:2]
        r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], SDMINL - 100)
        r["filled"] = orc.fill_occlusion(r["occlusion"], float(SDMINL))
        return r
    return solve


_LOOPS = {}


def _loop(orc, setting, init):
    """mi_ref.pair_loop of the scene (inverted right image, seed 0) over three tables, computed once"""
    key = (setting, init)
    if key not in _LOOPS:
        Il, Ir, truth, kept = ref.scene(0, "invert")
        _LOOPS[key] = (Il, Ir, truth, kept, ref.pair_loop(
            Il, Ir, SD, SDMINL, SDMINR, _solver(orc, Il, Ir, setting), 3, init, 0,
            lambda: (orc.cost_volume(Il, Ir, SD, SDMINL), orc.cost_volume(Ir, Il, SD, SDMINR))))
    return _LOOPS[key]


def _mp(iterations, init, seed=0):
    p = smx.default_mi_params()
    p.iterations, p.init, p.seed = iterations, init, seed
    return p


def _perm():
    p = smx.default_perm_params()
    p.sigma = SIGMA
    return p


@pytest.mark.parametrize("init", [ref.INIT_RANDOM, ref.INIT_REFERENCE], ids=["random", "reference"])
@pytest.mark.parametrize("setting", SETTINGS)
def test_pipeline_and_context_run_the_loop(orc, setting, init):
    from stereo_matching_cuda_amd.device import PairPipeline
    L = smx.lib()
    Il, Ir, truth, kept, passes = _loop(orc, setting, init)
    kw = {"sgm": dict(aggregation="sgm"), "permeability": dict(permeability=_perm()), "guided": {}}[setting]
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), SW, SH, SD, C.byref(ctx)))
    try:
        if setting == "sgm":
            _lib.check(L.smx_ctx_set_aggregation(ctx, 1, None))
        if setting == "permeability":
            _lib.check(L.smx_ctx_set_permeability(ctx, C.byref(_perm())))
        names = dict(best_l="bestl", best_r="bestr", dmap_l="dmapl", dmap_r="dmapr", occlusion="occlusion", filled="filled")

        def run():
            bufs = {k: np.empty((SH, SW), F32) for k in names}
            out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
            _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR, C.byref(out)))
            return bufs

        for iterations in (1, 3):
            want = passes[iterations - 1]
            pipe = PairPipeline(SW, SH, SD, dminl=SDMINL, dminr=SDMINR, cost="mi", mi_params=_mp(iterations, init), **kw)
            pipe.run(_t(Il), _t(Ir))
            got = pipe.results()
            for k in MAPS:
                _eq(got[k], want[k], f"{setting} pipeline, {iterations} tables: {k}")
            _eq(pipe.mi_hist.cpu().numpy().view(np.uint32), want["hist"], "the last histogram")
            _eq(pipe.mi_table.cpu().numpy(), want["table"], "the last table")
            _lib.check(L.smx_ctx_set_mi(ctx, C.byref(_mp(iterations, init))))
            first = run()
            for k, n in names.items():
                _eq(first[k], want[n], f"{setting} context, {iterations} tables: {k}")
            again = run()
            for k in names:
                _eq(again[k], first[k], f"{setting} context, the same pair again: {k}")
        if setting == "guided" and init == ref.INIT_RANDOM:
            # what the feature is for, on the GPU's own maps
            assert ref.wrong(first["dmap_l"], truth, kept) <= 73
    finally:
        L.smx_destroy(ctx)


def test_context_setter_volumes_and_refusals(orc):
    L = smx.lib()
    Il, Ir, truth, kept, passes = _loop(orc, "guided", ref.INIT_RANDOM)
    plain = orc.stereo_pair(Il, Ir, SD, dminl=SDMINL, dminr=SDMINR)
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), SW, SH, SD, C.byref(ctx)))
    try:
        for bad in (_mp(0, 0), _mp(17, 0), _mp(3, 2)):
            assert L.smx_ctx_set_mi(ctx, C.byref(bad)) == -1
        _lib.check(L.smx_ctx_set_mi(ctx, C.byref(_mp(3, 0))))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR) == -1
        msg = L.smx_last_error()
        assert b"mutual-information" in msg and b"smx_ctx_set_mi" in msg and b"census" not in msg
        # the volumes are the last pass's
        bufs = {k: np.empty((SD, SH, SW), F32) for k in ("cost_l", "cost_r")}
        bufs["filled"] = np.empty((SH, SW), F32)
        out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR, C.byref(out)))
        T = passes[2]["table"]
        _eq(bufs["cost_l"], ref.cost(T, Il, Ir, SD, SDMINL), "cost_l")
        _eq(bufs["cost_r"], ref.cost(T, Il, Ir, SD, SDMINR, right=True), "cost_r")
        _eq(bufs["filled"], passes[2]["filled"], "filled")
        # PatchMatch stereo keeps no cost volume
        _lib.check(L.smx_ctx_set_patchmatch(ctx, C.byref(smx.default_pm_params())))
        out2 = _lib.PairOut(filled=bufs["filled"].ctypes.data)
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR, C.byref(out2)) == -1
        assert b"mutual-information" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_patchmatch(ctx, None))
        # a later smx_ctx_set_cost replaces it: the plain pair again
        _lib.check(L.smx_ctx_set_cost(ctx, _lib.COST_MODES["reference"], None))
        maps = {k: np.empty((SH, SW), F32) for k in ("best_l", "dmap_l", "dmap_r", "occlusion", "filled")}
        out3 = _lib.PairOut(**{k: v.ctypes.data for k, v in maps.items()})
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR, C.byref(out3)))
        for k, n in (("best_l", "bestl"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"), ("occlusion", "occlusion"), ("filled", "filled")):
            _eq(maps[k], plain[n], f"reference again: {k}")
        _lib.check(L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR))
        _lib.check(L.smx_ctx_wait(ctx, None, None))
        # NULL switches it off, and leaves another cost alone
        _lib.check(L.smx_ctx_set_mi(ctx, C.byref(_mp(1, 1))))
        _lib.check(L.smx_ctx_set_mi(ctx, None))
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, SDMINL, SDMINR, C.byref(out3)))
        _eq(maps["filled"], plain["filled"], "off again")
    finally:
        L.smx_destroy(ctx)


def test_pipeline_refuses():
    from stereo_matching_cuda_amd.device import PairPipeline
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, cost="mi", aggregation="patchmatch")
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, cost="mi", s_begin=0, s_end=D // 2)
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, mi_params=smx.default_mi_params())
    with pytest.raises(ValueError):
        PairPipeline(W, H, D, cost="mi", mi_params=_mp(17, 0))


def test_the_default_cost_allocates_nothing_for_it():
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(W, H, D)
    assert pipe.cost is None and pipe.mi_hist is None and pipe.mi_table is None and pipe.mi_params is None
