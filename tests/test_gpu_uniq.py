"""Uniqueness filtering on the GPU (smx_dev_aggregate_wta_pair_uq, smx_dev_sgm_wta_pair_uq, smx_dev_uniqueness,
PairPipeline(uniqueness=...)), bit-exact against tests/uniq_ref.py.

The state of a run is checked against uniq_ref.second_best -- sec BY THE DEFINITION from the final winner -- over the real
aggregated volume q: the one the same call returns in d_agg (the natural-order passes read it back), or, for the passes over
the walkers' own scratch (comb order), the volume of a separate plain run with d_agg.  Keys must equal the plain call's and
the neighbour state the _nbr call's, bit for bit.

Run on the GPU box:  python -m pytest tests -m gpu -q -k uniq
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import sgm_ref
import speckle_ref
import uniq_ref as ref
from guarded import Guarded
from test_gpu_subpix import _Path, _eq, _pipe

pytestmark = pytest.mark.gpu

F32 = np.float32
RATIO = 0.25
IDENT = ref.IDENT


def _params(radius=9):
    p = smx.default_params()
    p.radius = radius
    return p


def _check_uq(uq, vols, s_begin=0, s_end=None, name=""):
    """uq (2, 3, h, w) against the definition over vols[v][D][h][w]; -> per view (z, c0, sec, zsec)"""
    out = []
    for v in range(2):
        z, c0, sec, rest, last, zsec = ref.second_best(vols[v], s_begin, s_end)
        _eq(uq[v, 0], sec, f"{name} view {v} sec")
        _eq(uq[v, 1], rest, f"{name} view {v} rest")
        _eq(uq[v, 2], last, f"{name} view {v} last")
        out.append((z, c0, sec, zsec))
    return out


def _triple(Il, Ir, D, want_nbr=True, **kw):
    """The plain run with d_agg (the reference volume and keys), the _nbr run, and the _uq runs without and with d_agg, with and
    without d_nbr: every uq run's keys / nbr / agg equal the others' and its state the definition's."""
    plain = _pipe(Il, Ir, D, want_agg=True, **kw)
    r = plain.results()
    vols = (r["aggl"], r["aggr"])
    keys = plain.keys.cpu().numpy()
    nbr = _pipe(Il, Ir, D, subpixel="parabola", **kw).nbr.cpu().numpy() if want_nbr else None
    stats = None
    for want_agg in (False, True):
        for sub in ((None, "parabola") if want_nbr else (None,)):
            name = f"uq agg={want_agg} nbr={sub}"
            u = _pipe(Il, Ir, D, uniqueness=RATIO, subpixel=sub, want_agg=want_agg, **kw)
            u.check_status()
            _eq(u.keys.cpu().numpy(), keys, name + " keys")
            if sub:
                _eq(u.nbr.cpu().numpy(), nbr, name + " nbr")
            if want_agg:
                ur = u.results()
                _eq(ur["aggl"], vols[0], name + " aggl")
                _eq(ur["aggr"], vols[1], name + " aggr")
            stats = _check_uq(u.uq.cpu().numpy(), vols, name=name)
    return vols, keys, stats


# ---------------------------------------------------------------------------------------------
# aggregation: paths, shapes, chunking
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,radius", [(0, 9), (1, 9), (1, 12), (0, 12), (3, 9), (3, 4), (5, 9), (4, 9)])
def test_every_path(path, radius):
    Il, Ir = synth.gen_pair(129, 70, 17, 7)
    with _Path(path):
        _triple(Il, Ir, 17, params=_params(radius), slices_in_flight=7, multi_kernel=path in (0, 1))
        want = {0: 5 if radius == 9 else 1, 3: 2}.get(path, path)
        assert smx.lib().smx_last_agg_path() == want


def _strip():
    s, b, t = C.c_int(), C.c_int(), C.c_int()
    _lib.check(smx.lib().smx_agg_geometry(9, C.byref(s), C.byref(b), C.byref(t)))
    return s.value


@pytest.mark.parametrize("shape", ["129x70", "19x41", "64x9", "2x1", "strip x3", "strip+1 x3", "strip+1 x4"])
@pytest.mark.parametrize("D", [1, 2, 3, 9, 17])
def test_shapes_and_the_unroll_tail(shape, D):
    """one strip and one strip plus one column; w no multiple of 4; odd h; odd w*h (natural, one pixel per lane) and even
    (two); D around the pass's unroll of 8"""
    w, h = {"strip x3": (_strip(), 3), "strip+1 x3": (_strip() + 1, 3), "strip+1 x4": (_strip() + 1, 4)}.get(shape) or \
        tuple(int(t) for t in shape.split("x"))
    Il, Ir = synth.gen_pair(w, h, D, 100 + D)
    _triple(Il, Ir, D, want_nbr=D in (3, 17))


@pytest.mark.parametrize("path", [5, 3, 1])
@pytest.mark.parametrize("msl", [0, 1, 2, 3, 5])
def test_chunking(path, msl):
    """D = 11 in launches of 11 | 1 x 11 | 2 .. | 3, 3, 3, 2 | 5, 5, 1 slices: the state crosses every kind of seam"""
    Il, Ir = synth.gen_pair(19, 41, 11, 3)
    with _Path(path):
        _triple(Il, Ir, 11, slices_in_flight=msl or None, multi_kernel=path == 1)


def test_split_calls_and_poisoned_state():
    """Two calls over [0, 9) and [9, 17) on one set of keys; the first with fresh keys on poisoned keys and state."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    D = 17
    Il, Ir = synth.gen_pair(153, 5, D, 1535)
    vols = _pipe(Il, Ir, D, want_agg=True).results()
    vols = (vols["aggl"], vols["aggr"])
    h, w = Il.shape
    L = smx.lib()
    tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    for path in (5, 3):
        for sub in (None, "parabola"):
            pipe = PairPipeline(w, h, D, slices_in_flight=7, uniqueness=RATIO, subpixel=sub)
            pipe.keys.fill_(0)                          # (loaded, a key of 0 would beat every winner)
            pipe.uq.fill_(float("nan"))
            pipe.uq[:, 0].fill_(-1e30)
            with _Path(path):
                for i, (s0, s1) in enumerate(((0, 9), (9, 17))):
                    L.smx_set_keys_fresh(1 if i == 0 else 0)
                    try:
                        pipe._aggregate_call(L.smx_dev_aggregate_wta_pair_uq, p(tl), p(tr), None, None, w, h, pipe.dminl,
                                             pipe.dminr, s0, s1, p(pipe.keys), None, None, p(pipe.ws), pipe.ws_bytes,
                                             p(pipe.nbr), p(pipe.uq))
                    finally:
                        L.smx_set_keys_fresh(0)
            pipe.check_status()
            _check_uq(pipe.uq.cpu().numpy(), vols, name=f"split calls path {path} nbr {sub}")


# ---------------------------------------------------------------------------------------------
# costs: materialised reference costs, the queued fall-back, census
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [False, True], ids=["clean", "minus-zero"])
def test_cost_volumes_and_the_queued_fallback(bad):
    import oracle
    D, w, h = 17, 160, 40
    dminl, dminr = -(D - 1), 2
    Il, Ir = synth.gen_pair(w, h, D, 3)
    cl = oracle.cost_volume(Il, Ir, D, dminl)
    cr = oracle.cost_volume(Ir, Il, D, dminr)
    if bad:
        cl[15, 7, 23] = -0.0                            # one value the comb walker's check refuses: the ring walker reruns
    for sub in (None, "equiangular"):
        plain = _pipe(Il, Ir, D, dminl=dminl, dminr=dminr, costs=(cl, cr), slices_in_flight=7, want_agg=True)
        r = plain.results()
        u = _pipe(Il, Ir, D, dminl=dminl, dminr=dminr, costs=(cl, cr), slices_in_flight=7, uniqueness=RATIO, subpixel=sub)
        assert smx.lib().smx_last_agg_path() == 5
        rr = C.c_int(-1)
        _lib.check(smx.lib().smx_dev_agg_fallback(C.c_void_p(u.ws.data_ptr()), C.byref(rr)))
        assert rr.value == int(bad)
        u.check_status()
        _eq(u.keys.cpu().numpy(), plain.keys.cpu().numpy(), "keys")
        _check_uq(u.uq.cpu().numpy(), (r["aggl"], r["aggr"]), name=f"costs bad={bad} nbr={sub}")


def test_census_costs_and_their_ties():
    """Census costs are small integers: exact ties are frequent, so every case of the recurrence occurs on real q."""
    D = 17
    Il, Ir = synth.gen_pair(129, 70, D, 5)
    Il[:, 40:90] = 77           # a textureless patch in both views: its codes are 0, so many slices cost exactly 0 there and
    Ir[:, 40:90] = 77           # the aggregated costs tie exactly, far apart too
    vols, keys, stats = _triple(Il, Ir, D, cost="census", slices_in_flight=5)
    z, c0, sec, zsec = stats[0]
    has = z >= 0
    chunk_last = has & ((z % 5 == 4) | (z == D - 1))
    chunk_first = has & (z % 5 == 0)
    for name, count in (("winner on a chunk's last slice", chunk_last.sum()), ("winner on a chunk's first slice", chunk_first.sum()),
                        ("sec before the winner", (has & (zsec >= 0) & (zsec < z)).sum()),
                        ("sec after the winner", (has & (zsec > z)).sum()),
                        ("tie two or more slices away", (has & (zsec >= 0) & (sec == c0)).sum())):
        assert count > 0, name
    assert (has & np.isposinf(sec)).sum() == 0          # (17 finite slices: every winner has a far slice) ...
    # ... so the pixels with sec = +inf come from a run of the same scene over two slices: no slice is two away
    _, _, stats2 = _triple(Il, Ir, 2, want_nbr=False, cost="census")
    z2, _, sec2, _ = stats2[0]
    assert ((z2 >= 0) & np.isposinf(sec2)).sum() == z2.size


# ---------------------------------------------------------------------------------------------
# memory contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [5, 3, 1])
def test_memory_contract(path):
    """Guard bands around d_uq, d_nbr and the keys; a poisoned d_uq with fresh keys; a poisoned, misaligned workspace."""
    import torch
    D, w, h = 9, 129, 7
    n = w * h
    Il, Ir = synth.gen_pair(w, h, D, 9)
    L = smx.lib()
    with _Path(path):
        vols = _pipe(Il, Ir, D, want_agg=True, multi_kernel=path == 1).results()
        ws_bytes = 2 * int(L.smx_agg_workspace_bytes(w, h, D))
        img = [Guarded(n, np.uint8, (h, w), plane=n).load(a) for a in (Il, Ir)]
        keys = Guarded(2 * n * 8, np.int64, (2, h, w), plane=n, fill=0x11)
        uq = Guarded(6 * n * 4, F32, (2, 3, h, w), plane=n, misalign=4, fill=0xFF)      # (0xFFFFFFFF: a NaN)
        nbr = Guarded(6 * n * 4, F32, (2, 3, h, w), plane=n, misalign=8)
        ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), misalign=13, fill=0x5A, plane=n)
        ws.view.fill_(0xC3)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = smx.default_params()
        L.smx_set_keys_fresh(1)
        try:
            rc = L.smx_dev_aggregate_wta_pair_uq(C.byref(p), img[0].ptr, img[1].ptr, None, None, w, h, -(D - 1), 0, 0, D, keys.ptr,
                                                 None, None, ws.ptr, ws_bytes, nbr.ptr, uq.ptr, st)
        finally:
            L.smx_set_keys_fresh(0)
        _lib.check(rc)
        for g, name in ((keys, "d_keys"), (uq, "d_uq"), (nbr, "d_nbr"), (ws, "d_workspace")):
            g.check(name)
        for g in img:
            g.check_unchanged("image")
        _lib.check(L.smx_dev_agg_status(ws.ptr))
        _check_uq(uq.numpy(), (vols["aggl"], vols["aggr"]), name=f"guarded path {path}")


# ---------------------------------------------------------------------------------------------
# SGM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("w,h,D", [(1, 1, 1), (1, 7, 2), (7, 1, 3), (64, 4, 64), (63, 5, 65), (33, 6, 256)])
def test_sgm(w, h, D, paths):
    import torch
    n = w * h
    rng = np.random.default_rng(w * 1000 + D)
    costs = [rng.integers(0, 63, (D, h, w)).astype(F32) for _ in range(2)]
    sp = _lib.SgmParams()
    sp.p1, sp.p2, sp.paths = 10, 120, paths
    L = smx.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for views in ((0, 1), (0,), (1,)):
        inp = [Guarded(c.nbytes, F32, c.shape, plane=n).load(c) if v in views else None for v, c in enumerate(costs)]
        nv = len(views)
        keys = Guarded(nv * n * 8, np.int64, (nv, h, w), plane=n)
        agg = Guarded(nv * D * n * 4, F32, (nv, D, h, w), plane=n)
        nbr = Guarded(nv * 3 * n * 4, F32, (nv, 3, h, w), plane=n)
        uq = Guarded(nv * 3 * n * 4, F32, (nv, 3, h, w), plane=n, misalign=4)
        ws_bytes = L.smx_sgm_workspace_bytes(w, h, D, nv)
        ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), misalign=13, fill=0x5A, plane=n)
        ws.view.fill_(0xC3)
        ptr = lambda g: None if g is None else g.ptr
        _lib.check(L.smx_dev_sgm_wta_pair_uq(C.byref(sp), ptr(inp[0]), ptr(inp[1]), w, h, D, keys.ptr, agg.ptr, nbr.ptr, uq.ptr,
                                             ws.ptr, ws_bytes, st))
        for g, name in ((keys, "d_keys"), (agg, "d_agg"), (nbr, "d_nbr"), (uq, "d_uq"), (ws, "d_ws")):
            g.check(name)
        for slot, v in enumerate(views):
            want = sgm_ref.outputs(costs[v], sp.p1, sp.p2, sp.paths)
            _eq(agg.numpy()[slot], want["agg"], "S")
            _eq(keys.numpy()[slot], want["keys"], "keys")
            _eq(nbr.numpy()[slot], want["nbr"], "nbr")
            z, c0, sec, rest, last, _ = ref.second_best(want["agg"])
            for k, plane in enumerate((sec, rest, last)):
                _eq(uq.numpy()[slot, k], plane, f"sgm {w}x{h}x{D} views {views} uq[{k}]")


# ---------------------------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------------------------
def _synthetic_state(h, w, seed):
    rng = np.random.default_rng(seed)
    c0s = np.array([0.0, -0.0, 1.0, -1.0, 4.0, -4.0, 100.0, 1e-30, np.inf, -np.inf], F32)
    secs = np.array([0.0, 1.0, 4.0, 4.5, 5.0, 6.0, -3.0, -4.0, 100.0, 124.0, 125.0, np.inf, -np.inf, np.nan], F32)
    disps = np.array([-15.0, -3.0, 0.0, -0.0, 2.5, -115.0, -16.0, -15.5, np.nan, np.inf, -np.inf, 3e9, -3e9], F32)
    c0 = c0s[rng.integers(0, c0s.size, (h, w))]
    keys = np.array([ref.pack_key(c, int(s)) for c, s in zip(c0.ravel(), rng.integers(0, 16, h * w))], np.int64).reshape(h, w)
    keys[rng.random((h, w)) < 0.1] = IDENT
    sec = secs[rng.integers(0, secs.size, (h, w))]
    disp = disps[rng.integers(0, disps.size, (h, w))]
    odd_nan = np.array([0xFFC00001, 0x7F800001], np.uint32).view(F32)           # NaNs with a payload: copied bit for bit
    disp.reshape(-1)[:min(2, h * w)] = odd_nan[:min(2, h * w)]
    return keys, sec, disp


@pytest.mark.parametrize("ratio", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("w,h", [(1, 1), (255, 3), (257, 5)])
def test_filter_rule(w, h, ratio):
    import torch
    n = w * h
    keys, sec, disp = _synthetic_state(h, w, w + h)
    has, c0 = ref.key_fields(keys)
    vmin, new_val = -15.0, -115.0
    want, want_m = ref.apply(disp, has, c0, sec, ratio, vmin, new_val)
    if ratio == 0:
        assert np.array_equal(want.view(np.uint32), disp.view(np.uint32))
    elif n > 1:
        assert (want.view(np.uint32) != disp.view(np.uint32)).any() and (ref.rejects(has, c0, sec, ratio) & ~ref.counts(disp, vmin)).any()
    L = smx.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gk = Guarded(n * 8, np.int64, (h, w), plane=n).load(keys)
    gs = Guarded(n * 4, F32, (h, w), plane=n, misalign=4).load(sec)               # (the sec plane alone: nothing more is read)
    for in_place in (False, True):
        for with_margin in (True, False):
            gd = Guarded(n * 4, F32, (h, w), plane=n).load(disp)
            go = Guarded(n * 4, F32, (h, w), plane=n, misalign=8)
            gm = Guarded(n * 4, F32, (h, w), plane=n, misalign=12)
            out = gd if in_place else go
            _lib.check(L.smx_dev_uniqueness(ratio, gk.ptr, gs.ptr, gd.ptr, out.ptr, gm.ptr if with_margin else None, w, h, vmin,
                                            new_val, st))
            assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))
            gk.check_unchanged("d_keys")
            gs.check_unchanged("d_uq")
            if in_place:
                go.check_untouched("d_out")
            else:
                gd.check_unchanged("d_disp")
            if with_margin:
                _eq(gm.numpy(), want_m, "margin")
            else:
                gm.check_untouched("d_margin")
    got, got_m = smx.uniqueness_filter(keys, sec, disp, ratio, vmin, new_val, want_margin=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    _eq(got_m, want_m, "host margin")


# ---------------------------------------------------------------------------------------------
# the pipeline
# ---------------------------------------------------------------------------------------------
def _chain(r, sec, pipe, speckle):
    """occlusion -> uniqueness -> speckle -> fill, in numpy"""
    import oracle
    has, c0 = ref.key_fields(pipe.keys[0].cpu().numpy())
    unique, margin = ref.apply(r["occlusion"], has, c0, sec, pipe.uniqueness, pipe.dminl, pipe.dminl - 100)
    kept = unique
    if speckle:
        kept = speckle_ref.speckle_filter(unique, float(pipe.dminl), float(pipe.dminl - 100), speckle.max_size, speckle.max_diff)
    return unique, margin, kept, oracle.fill_occlusion(kept, float(pipe.dminl))


def test_pipeline_alone_and_default_untouched():
    import torch
    import oracle
    D = 16
    Il, Ir = synth.gen_pair(129, 70, D, 21)
    base = _pipe(Il, Ir, D, want_agg=True)
    rb = base.results()
    assert base.uq is None and base.unique is None and base.margin is None
    off = _pipe(Il, Ir, D, uniqueness=None)
    for k, v in off.results().items():
        _eq(v, rb[k], "uniqueness=None " + k)
    want = oracle.stereo_pair(Il, Ir, D)
    for k in ("dmapl", "dmapr", "occlusion", "filled"):
        _eq(rb[k], want[k], "default " + k)
    pipe = _pipe(Il, Ir, D, uniqueness=RATIO)
    r = pipe.results()
    sec = ref.second_best(rb["aggl"])[2]
    _eq(pipe.uq[0, 0].cpu().numpy(), sec, "sec")
    unique, margin, kept, filled = _chain(r, sec, pipe, None)
    for k in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "meanl", "meanr"):
        _eq(r[k], rb[k], k)
    _eq(r["unique"], unique, "unique")
    _eq(r["margin"], margin, "margin")
    _eq(r["filled"], filled, "filled")
    assert (r["unique"] != r["occlusion"]).sum() > 0
    # two runs and a graph replay: the same bits
    tl, tr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        pipe.run(tl, tr)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pipe.run(tl, tr)
        for t in (pipe.unique, pipe.margin, pipe.filled, pipe.uq):
            t.zero_()
        g.replay()
    torch.cuda.current_stream().wait_stream(s)
    r2 = pipe.results()
    for k in r:
        _eq(r2[k], r[k], "replay " + k)
    with pytest.raises(ValueError):
        _pipe(Il, Ir, D, uniqueness=-1.0)


def test_pipeline_with_every_stage():
    import wmf_ref
    D = 16
    Il, Ir = synth.gen_pair(129, 70, D, 22)
    spk = _lib.SpeckleParams()
    spk.max_size, spk.max_diff = 30, 1.0
    kw = dict(cost="census", aggregation="sgm", subpixel="parabola", speckle=spk, wmf="occluded")
    base = _pipe(Il, Ir, D, want_agg=True, **kw)
    rb = base.results()
    pipe = _pipe(Il, Ir, D, uniqueness=RATIO, **kw)
    r = pipe.results()
    _eq(pipe.keys.cpu().numpy(), base.keys.cpu().numpy(), "keys")
    _eq(pipe.nbr.cpu().numpy(), base.nbr.cpu().numpy(), "nbr")
    sec = ref.second_best(rb["aggl"])[2]
    _eq(pipe.uq[0, 0].cpu().numpy(), sec, "sec")
    unique, margin, kept, filled = _chain(r, sec, pipe, spk)
    _eq(r["occlusion"], rb["occlusion"], "occlusion")
    _eq(r["unique"], unique, "unique")
    _eq(r["margin"], margin, "margin")
    _eq(r["despeckled"], kept, "despeckled")
    _eq(r["filled"], filled, "filled")
    import subpix_ref
    keep = subpix_ref.kept(kept, pipe.dminl)
    _eq(r["subpix_filled"], np.where(keep, r["subpixl"], filled).astype(F32), "sub_filled")
    _eq(r["refined"], wmf_ref.weighted_median(Il, filled, pipe.dminl, D, select=kept, radius=pipe.wmf_params.radius), "refined")
    assert (r["unique"] != r["occlusion"]).sum() > 0


def test_pipeline_refuses_a_slice_sub_range():
    from stereo_matching_cuda_amd.device import PairPipeline
    with pytest.raises(ValueError):
        PairPipeline(64, 9, 16, uniqueness=RATIO, s_begin=0, s_end=8)
    with pytest.raises(ValueError):
        PairPipeline(64, 9, 16, uniqueness=RATIO, s_begin=8)


# ---------------------------------------------------------------------------------------------
# the persistent context
# ---------------------------------------------------------------------------------------------
CW, CH, CD = 129, 70, 16
#           census, sgm, subpixel, speckle
SETTINGS = [(False, False, False, False), (True, False, False, True), (True, True, True, True), (False, True, False, False),
            (False, False, True, True), (True, False, True, False)]


def _spk():
    s = _lib.SpeckleParams()
    s.max_size, s.max_diff = 30, 1.0
    return s


def _ctx_run(L, ctx, Il, Ir, ratio, census, sgm, subpixel, speckle, want_cost=False):
    """One synchronous pair on `ctx` with these settings -> {name: array}; want_cost: the caller asks for the cost volumes,
    which sends the census cost through the context's whole-volume loop instead of its chunk loop"""
    n = CW * CH
    _lib.check(L.smx_ctx_set_cost(ctx, 1 if census else 0, None))
    _lib.check(L.smx_ctx_set_aggregation(ctx, 1 if sgm else 0, None))
    _lib.check(L.smx_ctx_set_subpixel(ctx, 1 if subpixel else 0))
    _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(_spk()) if speckle else None))
    _lib.check(L.smx_ctx_set_uniqueness(ctx, ratio))
    bufs = {k: np.empty((CH, CW), F32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if want_cost:
        bufs["cost_l"], bufs["cost_r"] = np.empty((CD, CH, CW), F32), np.empty((CD, CH, CW), F32)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, -(CD - 1), 0, C.byref(out)))
    r = {"bestl": bufs["best_l"], "bestr": bufs["best_r"], "dmapl": bufs["dmap_l"], "dmapr": bufs["dmap_r"],
         "occlusion": bufs["occlusion"], "filled": bufs["filled"]}
    if ratio > 0:
        r["unique"], r["margin"] = np.empty((CH, CW), F32), np.empty((CH, CW), F32)
        _lib.check(L.smx_ctx_uniqueness_map(ctx, r["unique"].ctypes.data, r["margin"].ctypes.data))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, -(CD - 1), 0) == -1
        if not (census or sgm or subpixel or speckle):          # (else another stage's refusal comes first)
            assert b"smx_ctx_set_uniqueness" in L.smx_last_error()
    else:
        assert L.smx_ctx_uniqueness_map(ctx, None, None) == -1
    if speckle:
        r["despeckled"] = np.empty((CH, CW), F32)
        _lib.check(L.smx_ctx_speckle_map(ctx, r["despeckled"].ctypes.data))
    if subpixel:
        sub = [np.empty((CH, CW), F32) for _ in range(3)]
        _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
        r["subpixl"], r["subpixr"], r["subpix_filled"] = sub
    return r


def test_context_equals_the_pipeline_and_toggles_cleanly():
    """The context entry against PairPipeline (itself held to the numpy chain above) in every combination of the census cost
    (chunked and whole-volume loops), SGM, sub-pixel and speckle; ONE context toggled through all settings, the filter on
    and off in turn, against a fresh context per setting, bit for bit."""
    Il, Ir = synth.gen_pair(CW, CH, CD, 23)
    L = smx.lib()
    P = smx.default_params()
    one = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), CW, CH, CD, C.byref(one)))
    try:
        for bad in (float("nan"), -1.0, float("inf")):
            assert L.smx_ctx_set_uniqueness(one, bad) == -1
        changed = 0
        for census, sgm, subpixel, speckle in SETTINGS:
            for ratio in (RATIO, 0.0):
                name = f"census={census} sgm={sgm} subpixel={subpixel} speckle={speckle} ratio={ratio}"
                got = _ctx_run(L, one, Il, Ir, ratio, census, sgm, subpixel, speckle)
                if census and not sgm:
                    whole = _ctx_run(L, one, Il, Ir, ratio, census, sgm, subpixel, speckle, want_cost=True)
                    for k in got:
                        _eq(whole[k], got[k], f"whole-volume census loop, {name}: {k}")
                fresh = C.c_void_p()
                _lib.check(L.smx_create(C.byref(P), CW, CH, CD, C.byref(fresh)))
                try:
                    want = _ctx_run(L, fresh, Il, Ir, ratio, census, sgm, subpixel, speckle)
                finally:
                    L.smx_destroy(fresh)
                assert got.keys() == want.keys()
                for k in got:
                    _eq(got[k], want[k], f"toggled context, {name}: {k}")
                pipe = _pipe(Il, Ir, CD, uniqueness=ratio or None, cost="census" if census else None,
                             aggregation="sgm" if sgm else None, subpixel="parabola" if subpixel else None,
                             speckle=_spk() if speckle else None)
                pr = pipe.results()
                for k in got:
                    _eq(got[k], pr[k], f"context against pipeline, {name}: {k}")
                if ratio:
                    changed += int((got["unique"] != got["occlusion"]).sum())
        assert changed > 0
    finally:
        L.smx_destroy(one)
