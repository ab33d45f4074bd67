"""The information permeability filter on the GPU (csrc/smx_perm.hip), bit for bit against tests/perm_ref.py:
  smx_dev_permeability_wta_pair  random f32 volumes with ties, NaN, -0 and infinities planted -- no aggregation involved -- over
                                 the shapes of the issue and one on each side of every gate the kernels have (below), size_d 1 /
                                 3 / 17, 1 / 3 / 4 channels, one and two views, out NULL / separate / in place, the four state
                                 combinations, one chunk of slices against several; every buffer in a Guarded, the workspace
                                 poisoned with NaN bits
  the context, PairPipeline      the aggregated volumes come from the oracle (reference cost, gray guide) or from plain pipelines
                                 (census, AD-Census, colour guide: the existing entries, held to their own references elsewhere),
                                 the filter, the winners and everything behind them from the numpy references

The kernels' gates: the horizontal pass takes 64 rows a wave (h of 64 / 65) and walks them in tiles of 32 columns (w of 32 /
33 and 64 / 65); the vertical pass takes 256 columns a workgroup (w of 256 / 257) and walks the rows in batches of 8 (h of 8 /
9).  There is no LDS-staged size limit and no vector width to choose: every access is a 4-byte one.

A NaN carries no agreed payload: two values are "the same bits" here if they are both NaN or have equal bits.

Run on the GPU box:  python -m pytest tests -m gpu -q -k perm
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import adjust_ref
import perm_ref as ref
import subpix_ref
import uniq_ref
from guarded import SMX_E_WS, Guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
PRESET = np.uint32(0x7F7F7F7F).view(F32)


def same(a, b, name):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == F32:
        nan = np.isnan(a) & np.isnan(b)
        bad = np.flatnonzero(((a.view(np.uint32) != b.view(np.uint32)) & ~nan).ravel())
    else:
        bad = np.flatnonzero((a != b).ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} differ, first at {bad[:5]}: {a.ravel()[bad[:5]]} != {b.ravel()[bad[:5]]}"


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(sigma):
    p = smx.default_perm_params()
    p.sigma = sigma
    return p


# ---------------------------------------------------------------------------------------------
# host entries that need no device
# ---------------------------------------------------------------------------------------------
def test_defaults_and_table_equal_the_reference():
    L = smx.lib()
    assert smx.default_perm_params().sigma == 32.0 == ref.DEFAULT_SIGMA
    for sigma in (32.0, 16.0, 64.0, 0.001, 0.011, 0.012, 1e6, 7.3):
        got = np.array(smx.perm_table(_params(sigma)), F32)
        same(got, ref.table(sigma), f"table {sigma}")
        assert got[0] == 1.0
    t = (C.c_float * 256)()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.smx_perm_table(C.byref(_params(bad)), t) == -1 and b"sigma" in L.smx_last_error()
    assert L.smx_perm_workspace_bytes(19, 40, 17, 2) == 2 * 19 * 40 * 4 * (2 + 2 * 17)
    for bad in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, 0, 1), (4, 4, 1, 0), (4, 4, 1, 3), (1 << 16, 1 << 15, 1, 1)):
        assert L.smx_perm_workspace_bytes(*bad) == 0


# ---------------------------------------------------------------------------------------------
# the filter and its winner-take-all pass on random volumes
# ---------------------------------------------------------------------------------------------
def _volume(rng, w, h, size_d, smooth):
    """a view's volume: few distinct values (ties) or normal ones, -0 in many places.  A NaN or an infinity reaches its whole
    row in the horizontal pass (0 * inf is a NaN too) and from there every column: it takes its slice with it.  So one slice
    gets a NaN, one a +inf and one a -inf where there are four, so that most slices stay finite; with fewer slices every other
    volume carries one."""
    v = (rng.integers(-3, 4, (size_d, h, w)) * 0.5).astype(F32) if smooth else rng.standard_normal((size_d, h, w)).astype(F32)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = -0.0
    specials = (np.nan, np.inf, -np.inf) if size_d >= 4 else (np.nan, np.inf)[:size_d - 1] if smooth else ()
    for z, val in zip(rng.permutation(size_d), specials):
        v[z, rng.integers(0, h), rng.integers(0, w)] = val
    return v


def _guide(rng, w, h, ch):
    """flat patches with a few edges: permeabilities of 1, of small steps and of hard edges"""
    base = rng.integers(0, 256, (h // 7 + 1, w // 5 + 1, ch)).astype(np.int64)
    g = np.kron(base, np.ones((7, 5, 1), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w, ch))
    g = np.clip(g, 0, 255).astype(np.uint8)
    return g[:, :, 0] if ch == 1 else g


def _want_view(vol, guide, sigma):
    out = ref.filter_volume(vol, guide, sigma)
    z, c0, lo, hi, last = subpix_ref.winners(out)
    _, _, sec, rest, last_u, _ = uniq_ref.second_best(out)
    return dict(out=out, keys=ref.pack_keys(z, c0), nbr=np.stack([lo, hi, last]).astype(F32),
                uq=np.stack([sec, rest, last_u]).astype(F32))


FORMS = list(itertools.product(("both", "left", "right"), ("none", "separate", "in place"), (False, True), (False, True)))


def _call(vols, guides, wants, w, h, size_d, sigma, views, store, nbr, uq, ws_slices=None, expect=0):
    """one smx_dev_permeability_wta_pair on guarded buffers; checks everything it wrote and everything it must not write.
    ws_slices: the slices in flight the workspace is sized for (None: all of them); expect: the return code"""
    L = smx.lib()
    n = w * h
    used = [0, 1] if views == "both" else [0] if views == "left" else [1]
    V = len(used)
    ch = 1 if guides[0].ndim == 2 else guides[0].shape[2]
    name = f"{w}x{h} D {size_d} ch {ch} sigma {sigma} {views} out {store} nbr {nbr} uq {uq} ws for {ws_slices}"
    vin = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), plane=n).load(np.stack([vols[v] for v in used]))
    gd = [Guarded(guides[v].nbytes, np.uint8, guides[v].shape, plane=n).load(guides[v]) for v in used]
    keys = Guarded(V * n * 8, np.int64, (V, h, w), plane=n, fill=0x11)
    out = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), plane=n) if store == "separate" else None
    gn = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if nbr else None
    gu = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if uq else None
    per = V * n * 4
    k = size_d if ws_slices is None else ws_slices
    ws_bytes = per * (2 + k * (2 if store == "none" else 1)) if k else per * (3 if store == "none" else 2) + per - 4
    ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), plane=n, fill=0xFF)
    ptrs = [None, None], [None, None]
    for i, v in enumerate(used):
        ptrs[0][v] = C.c_void_p(vin.ptr.value + i * size_d * n * 4)
        ptrs[1][v] = gd[i].ptr
    d_out = vin.ptr if store == "in place" else out.ptr if out else None
    rc = L.smx_dev_permeability_wta_pair(C.byref(_params(sigma)), ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1], ch, w, h, -3, 2,
                                         size_d, keys.ptr, d_out, gn.ptr if gn else None, gu.ptr if gu else None, ws.ptr, ws_bytes,
                                         _stream())
    assert rc == expect, (name, rc, L.smx_last_error())
    for g in gd:
        g.check_unchanged(name + ": guide")
    if rc != 0:
        vin.check_unchanged(name + ": volume of a refused call")
        for g, what in ((keys, "keys"), (out, "out"), (gn, "nbr"), (gu, "uq"), (ws, "workspace")):
            if g is not None:
                g.check_untouched(f"{name}: {what} of a refused call")
        return None
    if store == "in place":
        vin.check(name + ": volume / out")
    else:
        vin.check_unchanged(name + ": volume")
    got_out = vin.numpy() if store == "in place" else out.numpy() if out else None
    for g, what in ((keys, "keys"), (out, "out"), (gn, "nbr"), (gu, "uq"), (ws, "workspace")):
        if g is not None:
            g.check(f"{name}: {what}")
    for i, v in enumerate(used):
        same(keys.numpy()[i], wants[v]["keys"], f"{name}: keys of view {v}")
        if got_out is not None:
            same(got_out[i], wants[v]["out"], f"{name}: out of view {v}")
        if gn:
            same(gn.numpy()[i], wants[v]["nbr"], f"{name}: nbr of view {v}")
        if gu:
            same(gu.numpy()[i], wants[v]["uq"], f"{name}: uq of view {v}")
    return dict(keys=keys.numpy(), out=got_out, nbr=gn.numpy() if gn else None, uq=gu.numpy() if gu else None)


# (w, h, the slice counts): the issue's shapes, then one on each side of every gate with at most two slices
SHAPES = [(1, 1, (1, 3, 17)), (2, 1, (1, 3, 17)), (1, 2, (1, 3, 17)), (19, 40, (1, 3, 17)), (64, 9, (1, 3, 17)), (65, 9, (1, 3, 17)),
          (129, 70, (1, 3, 17)), (210, 150, (1, 3, 17)), (9, 64, (2,)), (8, 65, (2,)), (32, 5, (2,)), (33, 3, (2,)), (256, 3, (2,)),
          (257, 8, (1,)), (513, 2, (2,))]


@pytest.mark.parametrize("w,h,slices", SHAPES)
def test_filter_and_winners(w, h, slices):
    rng = np.random.default_rng(w * 1000 + h)
    forms = itertools.cycle(FORMS[(7 * SHAPES.index((w, h, slices))) % len(FORMS):] + FORMS)
    sigmas = itertools.cycle((32.0, 4.0, 0.011, 200.0))
    for k, size_d in enumerate(slices):
        for ch in (1, 3, 4):
            sigma = next(sigmas)
            vols = [_volume(rng, w, h, size_d, smooth=(k + v) % 2 == 0) for v in range(2)]
            guides = [_guide(rng, w, h, ch) for _ in range(2)]
            wants = [_want_view(vols[v], guides[v], sigma) for v in range(2)]
            for _ in range(2 if len(slices) > 1 else 6):
                views, store, nbr, uq = next(forms)
                _call(vols, guides, wants, w, h, size_d, sigma, views, store, nbr, uq)


def test_every_form_on_one_shape():
    """all 36 combinations of views, output and states on 65 x 9 x 3"""
    w, h, size_d, sigma = 65, 9, 3, 32.0
    rng = np.random.default_rng(5)
    vols = [_volume(rng, w, h, size_d, smooth=v == 0) for v in range(2)]
    guides = [_guide(rng, w, h, 3) for _ in range(2)]
    wants = [_want_view(vols[v], guides[v], sigma) for v in range(2)]
    for views, store, nbr, uq in FORMS:
        _call(vols, guides, wants, w, h, size_d, sigma, views, store, nbr, uq)


@pytest.mark.parametrize("store", ["none", "separate", "in place"])
def test_chunks_of_slices_give_the_same_bits(store):
    """a workspace for 17 slices in flight (one chunk) against ones for 5, 2 and 1 (4, 9 and 17 chunks), and the calling
    thread's smx_set_max_slices_per_launch"""
    L = smx.lib()
    w, h, size_d, sigma = 70, 33, 17, 32.0
    rng = np.random.default_rng(17)
    vols = [_volume(rng, w, h, size_d, smooth=v == 0) for v in range(2)]
    guides = [_guide(rng, w, h, 1) for _ in range(2)]
    wants = [_want_view(vols[v], guides[v], sigma) for v in range(2)]
    whole = _call(vols, guides, wants, w, h, size_d, sigma, "both", store, True, True)
    for k in (5, 2, 1):
        part = _call(vols, guides, wants, w, h, size_d, sigma, "both", store, True, True, ws_slices=k)
        for name in whole:
            if whole[name] is not None:
                same(part[name], whole[name], f"{store}, {k} slices in flight: {name}")
    _lib.check(L.smx_set_max_slices_per_launch(3))
    try:
        _call(vols, guides, wants, w, h, size_d, sigma, "left", store, True, False)
    finally:
        _lib.check(L.smx_set_max_slices_per_launch(0))


@pytest.mark.parametrize("views,store", [("both", "none"), ("both", "in place"), ("left", "separate"), ("right", "none")])
def test_a_workspace_below_one_slice_is_refused_before_any_launch(views, store):
    """4 bytes short of one slice in flight: SMX_E_WS, and no buffer of the call -- the poisoned workspace included -- is touched"""
    w, h, size_d = 19, 40, 3
    rng = np.random.default_rng(3)
    vols = [_volume(rng, w, h, size_d, True) for _ in range(2)]
    guides = [_guide(rng, w, h, 1) for _ in range(2)]
    _call(vols, guides, None, w, h, size_d, 32.0, views, store, True, True, ws_slices=0, expect=SMX_E_WS)
    assert b"workspace" in smx.lib().smx_last_error()


def test_refused_arguments():
    L = smx.lib()
    g = Guarded(4096, F32, (1024,))
    ok = _params(32.0)
    v, odd = g.ptr, C.c_void_p(g.ptr.value + 2)
    tail = (g.ptr, None, None, None, g.ptr, 4096)
    calls = [(_params(0.0), v, None, v, None, 1, 4, 4, 0, 0, 2), (_params(float("nan")), v, None, v, None, 1, 4, 4, 0, 0, 2),
             (_params(float("inf")), v, None, v, None, 1, 4, 4, 0, 0, 2), (_params(-2.0), v, None, v, None, 1, 4, 4, 0, 0, 2),
             (ok, v, None, v, None, 2, 4, 4, 0, 0, 2), (ok, None, None, None, None, 1, 4, 4, 0, 0, 2),
             (ok, v, None, None, None, 1, 4, 4, 0, 0, 2), (ok, v, None, v, v, 1, 4, 4, 0, 0, 2), (ok, v, None, v, None, 1, 0, 4, 0, 0, 2),
             (ok, v, None, v, None, 1, 4, 0, 0, 0, 2), (ok, v, None, v, None, 1, 4, 4, 0, 0, 0),
             (ok, v, None, v, None, 1, 1 << 16, 1 << 15, 0, 0, 2), (ok, odd, None, v, None, 1, 4, 4, 0, 0, 2),
             (ok, v, None, v, None, 1, 4, 4, 1 << 30, 0, 2)]
    for c in calls:
        assert L.smx_dev_permeability_wta_pair(C.byref(c[0]), *c[1:], *tail, _stream()) == -1, c
        assert L.smx_last_error()
    # states without keys
    assert L.smx_dev_permeability_wta_pair(C.byref(ok), v, None, v, None, 1, 4, 4, 0, 0, 2, None, None, g.ptr, None, g.ptr, 4096,
                                           _stream()) == -1
    # no workspace
    assert L.smx_dev_permeability_wta_pair(C.byref(ok), v, None, v, None, 1, 4, 4, 0, 0, 2, g.ptr, None, None, None, None, 0,
                                           _stream()) == SMX_E_WS
    g.check_untouched("refused calls")


def test_host_entry():
    """stages.permeability_filter: an aggregated volume behind the guided filter, and the paper's own form on a raw cost volume"""
    import oracle
    w, h, size_d, dmin = 70, 20, 9, -8
    Il, Ir = synth.gen_pair(w, h, size_d, 77)
    r = oracle.stereo_pair(Il, Ir, size_d, dminl=dmin, dminr=0, want_cost=True, want_agg=True)
    for vol, sigma in ((r["aggl"], None), (r["costl"], 16.0), (r["aggl"], _params(8.0))):
        s = 32.0 if sigma is None else sigma.sigma if isinstance(sigma, _lib.PermParams) else sigma
        want = ref.filter_volume(vol, Il, s)
        z, c0 = ref.winners(want)
        out, best, disp = smx.permeability_filter(vol, Il, sigma, dmin=dmin)
        same(out, want, "host entry out")
        same(best, c0, "host entry best")
        same(disp, ref.label_map(z, dmin), "host entry labels")
    rgb = np.stack([Il, Il[::-1], Il[:, ::-1]], axis=2).copy()
    same(smx.permeability_filter(r["aggl"], rgb, 32.0)[0], ref.filter_volume(r["aggl"], rgb, 32.0), "host entry, colour guide")
    for bad in (0.0, float("nan"), -1.0):
        with pytest.raises(ValueError):
            smx.permeability_filter(r["aggl"], Il, bad)
    with pytest.raises(ValueError):
        smx.permeability_filter(r["aggl"], Il[:-1], 32.0)


# ---------------------------------------------------------------------------------------------
# the context and PairPipeline
# ---------------------------------------------------------------------------------------------
D, DMINL, DMINR = 16, -15, 0
W, H = 129, 70


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _images(w, h, guide, seed):
    """gray pair (and colour pair with the colour guide: the gray one is then the library's gray of it, as the context makes it)"""
    Il, Ir = synth.gen_pair(w, h, D, seed)
    if guide != "rgb":
        return (Il, Ir), None
    rng = np.random.default_rng(seed)
    rgb = tuple(np.clip(g[:, :, None].astype(np.int64) + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8) for g in (Il, Ir))
    return tuple(smx.rgb_to_grayscale(c) for c in rgb), rgb


def _adc():
    p = smx.default_adcensus_params()
    p.colour = 0
    return p


def _pipe_kw(cost, guide):
    kw = dict(cost=None if cost == "reference" else cost, guidance="rgb" if guide == "rgb" else None)
    if cost == "adcensus":
        kw["adcensus_params"] = _adc()
    return kw


def _plain_volumes(orc, gray, rgb, w, h, cost, guide):
    """both views' aggregated volumes WITHOUT the filter: the oracle's for the reference cost with the gray guide, else a plain
    pipeline's"""
    if cost == "reference" and guide == "gray":
        r = orc.stereo_pair(gray[0], gray[1], D, dminl=DMINL, dminr=DMINR, want_agg=True)
        return r["aggl"], r["aggr"]
    from stereo_matching_cuda_amd.device import PairPipeline
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, want_agg=True, **_pipe_kw(cost, guide))
    pipe.run(_t(gray[0]), _t(gray[1]), **(dict(rgb_l=_t(rgb[0]), rgb_r=_t(rgb[1])) if rgb else {}))
    r = pipe.results()
    return r["aggl"].copy(), r["aggr"].copy()


def _want_pair(orc, vols, guides, sigma, chain=None):
    """the pair's outputs from the plain volumes through the numpy references; chain: dict(mode, ratio, adjust) or None"""
    filt = [ref.filter_volume(vols[v], guides[v], sigma) for v in range(2)]
    win = [subpix_ref.winners(c) for c in filt]
    r = {"aggl": filt[0], "aggr": filt[1]}
    for v, side in enumerate("lr"):
        z, c0 = win[v][:2]
        took = (z >= 0) & (PRESET >= c0)
        r["dmap" + side] = subpix_ref.dmap_of(z, c0, (DMINL, DMINR)[v])
        r["best" + side] = np.where(took, c0, PRESET).astype(F32)
    r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], DMINL - 100)
    r["filled"] = orc.fill_occlusion(r["occlusion"], DMINL)
    if chain:
        z, c0, lo, hi, _ = win[0]
        sec = uniq_ref.second_best(filt[0])[2]
        r["unique"], r["margin"] = uniq_ref.apply(r["occlusion"], z >= 0, c0, sec, chain["ratio"], DMINL, DMINL - 100)
        filled = orc.fill_occlusion(r["unique"], DMINL)
        r["subpixl"], sub_filled = subpix_ref.maps(chain["mode"], z, c0, lo, hi, r["dmapl"], r["unique"], filled, DMINL)
        zr, cr, lor, hir, _ = win[1]
        r["subpixr"] = subpix_ref.maps(chain["mode"], zr, cr, lor, hir, r["dmapr"])[0]
        r["adjusted"], r["subpix_filled"] = adjust_ref.adjust(filled, filt[0], DMINL, mode=chain["mode"], sub=sub_filled,
                                                              **chain["adjust"])
        r["filled"] = r["adjusted"]
    return r


def _ctx_run(ctx, gray, rgb, w, h, want_vol=True):
    L = smx.lib()
    bufs = {k: np.empty((h, w), F32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if want_vol:
        bufs["agg_l"], bufs["agg_r"] = np.empty((D, h, w), F32), np.empty((D, h, w), F32)
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    if rgb:
        rc = L.smx_ctx_stereo_pair_rgb(ctx, rgb[0].ctypes.data, rgb[1].ctypes.data, 3, DMINL, DMINR, C.byref(out))
    else:
        rc = L.smx_ctx_stereo_pair(ctx, gray[0].ctypes.data, gray[1].ctypes.data, DMINL, DMINR, C.byref(out))
    return rc, bufs


def _ctx(w, h, cost, guide):
    L = smx.lib()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), w, h, D, C.byref(ctx)))
    if cost == "census":
        _lib.check(L.smx_ctx_set_cost(ctx, _lib.COST_MODES["census"], None))
    if cost == "adcensus":
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(_adc())))
    if guide == "rgb":
        _lib.check(L.smx_ctx_set_guidance(ctx, _lib.GUIDE_MODES["rgb"]))
    return ctx


CTX_NAMES = (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"), ("occlusion", "occlusion"),
             ("filled", "filled"), ("agg_l", "aggl"), ("agg_r", "aggr"))


@pytest.mark.parametrize("guide", ["gray", "rgb"])
@pytest.mark.parametrize("cost", ["reference", "census", "adcensus"])
def test_context_and_pipeline(orc, cost, guide):
    from stereo_matching_cuda_amd.device import PairPipeline
    L = smx.lib()
    w, h, sigma = W, H, 32.0
    gray, rgb = _images(w, h, guide, 31)
    vols = _plain_volumes(orc, gray, rgb, w, h, cost, guide)
    want = _want_pair(orc, vols, rgb if rgb else gray, sigma)
    kw = dict(rgb_l=_t(rgb[0]), rgb_r=_t(rgb[1])) if rgb else {}
    name = f"{cost} {guide}"
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, permeability=True, **_pipe_kw(cost, guide))
    pipe.run(_t(gray[0]), _t(gray[1]), **kw)
    got = pipe.results()
    for _, k in CTX_NAMES:
        same(got[k], want[k], f"{name} pipeline {k}")
    # the context: off, on (with and without the volumes fetched), off again
    ctx = _ctx(w, h, cost, guide)
    try:
        rc, off = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_permeability(ctx, C.byref(_params(sigma))))
        for want_vol in (True, False):
            rc, on = _ctx_run(ctx, gray, rgb, w, h, want_vol)
            _lib.check(rc)
            for k, n in CTX_NAMES[:8 if want_vol else 6]:
                same(on[k], want[n], f"{name} context {k}")
                same(on[k], got[n], f"{name} context against the pipeline {k}")
        _lib.check(L.smx_ctx_set_permeability(ctx, None))
        rc, again = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        for k, _ in CTX_NAMES:
            same(again[k], off[k], f"{name} context, off again {k}")
        same(off["agg_l"], vols[0], f"{name} context, plain volume")
        assert np.count_nonzero(want["dmapl"] != off["dmap_l"]) > 0          # (the filter does change winners here)
    finally:
        L.smx_destroy(ctx)


@pytest.mark.parametrize("mode", ["parabola", "equiangular"])
def test_the_stages_behind_run_on_the_filtered_volume(orc, mode):
    """sub-pixel + uniqueness + adjustment on: every output is the chain of the existing numpy references on the filtered
    volumes"""
    from stereo_matching_cuda_amd.device import PairPipeline
    L = smx.lib()
    w, h, sigma, ratio = W, H, 24.0, 0.05
    adj = dict(tau_e=2, vertical=1, iterations=2)
    gray, _ = _images(w, h, "gray", 11)
    vols = _plain_volumes(orc, gray, None, w, h, "reference", "gray")
    want = _want_pair(orc, vols, gray, sigma, dict(mode=subpix_ref.MODES[mode], ratio=ratio, adjust=adj))
    ap = smx.default_adjust_params()
    ap.tau_e, ap.vertical, ap.iterations = adj["tau_e"], adj["vertical"], adj["iterations"]
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, permeability=_params(sigma), subpixel=mode, uniqueness=ratio, adjust=ap)
    pipe.run(_t(gray[0]), _t(gray[1]))
    got = pipe.results()
    for k in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "unique", "margin", "filled", "adjusted", "subpixl", "subpixr",
              "subpix_filled", "aggl", "aggr"):
        same(got[k], want[k], f"pipeline {k}")
    ctx = _ctx(w, h, "reference", "gray")
    try:
        _lib.check(L.smx_ctx_set_permeability(ctx, C.byref(_params(sigma))))
        _lib.check(L.smx_ctx_set_subpixel(ctx, subpix_ref.MODES[mode]))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, ratio))
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(ap)))
        rc, on = _ctx_run(ctx, gray, None, w, h, want_vol=False)
        _lib.check(rc)
        for k, n in CTX_NAMES[:6]:
            same(on[k], want[n], f"context {k}")
        maps = [np.empty((h, w), F32) for _ in range(5)]
        _lib.check(L.smx_ctx_subpixel_maps(ctx, *[m.ctypes.data for m in maps[:3]]))
        _lib.check(L.smx_ctx_uniqueness_map(ctx, *[m.ctypes.data for m in maps[3:]]))
        for m, n in zip(maps, ("subpixl", "subpixr", "subpix_filled", "unique", "margin")):
            same(m, want[n], f"context {n}")
    finally:
        L.smx_destroy(ctx)


def _held(ctx):
    nbytes = C.c_size_t(1)
    _lib.check(smx.lib().smx_ctx_perm_held(ctx, C.byref(nbytes)))
    return nbytes.value


def test_a_context_without_the_setter_allocates_nothing_new():
    """Off by default: a context whose pairs never ran with the filter on holds no byte for it -- whether the setter was never
    called, or called and switched off again before the first pair (smx_ctx_perm_held: the workspace is all the feature
    allocates)."""
    L = smx.lib()
    (Il, Ir), _ = _images(W, H, "gray", 5)
    for prepare, expect in ((lambda c: None, 0),
                            (lambda c: (_lib.check(L.smx_ctx_set_permeability(c, C.byref(_params(32.0)))),
                                        _lib.check(L.smx_ctx_set_permeability(c, None))), 0),
                            (lambda c: _lib.check(L.smx_ctx_set_permeability(c, C.byref(_params(32.0)))), 2 * W * H * 4 * (2 + D))):
        ctx = _ctx(W, H, "reference", "gray")
        try:
            prepare(ctx)
            assert _held(ctx) == 0
            _lib.check(_ctx_run(ctx, (Il, Ir), None, W, H, want_vol=False)[0])
            assert _held(ctx) == expect
        finally:
            L.smx_destroy(ctx)


def test_refused_combinations():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    L = smx.lib()
    w, h = 40, 19
    for agg in ("sgm", "cross", "scanline", "cross-scanline", "patchmatch"):
        with pytest.raises(ValueError):
            PairPipeline(w, h, D, permeability=True, aggregation=agg)
    for bad in (dict(s_begin=1), dict(s_end=D - 1), dict(permeability=_params(0.0)), dict(permeability=_params(float("inf"))),
                dict(permeability=_params(float("nan"))), dict(permeability=32.0), dict(cross_scale=True)):
        with pytest.raises(ValueError):
            PairPipeline(w, h, D, **{"permeability": True, **bad})
    with pytest.raises(ValueError):
        ShardedPair(w, h, D, permeability=True)
    (Il, Ir), _ = _images(w, h, "gray", 1)
    ctx = _ctx(w, h, "reference", "gray")
    try:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert L.smx_ctx_set_permeability(ctx, C.byref(_params(bad))) == -1 and b"sigma" in L.smx_last_error()
        rc, plain = _ctx_run(ctx, (Il, Ir), None, w, h)                 # a refused setter leaves it off
        _lib.check(rc)
        assert _held(ctx) == 0
        _lib.check(L.smx_ctx_set_permeability(ctx, C.byref(_params(32.0))))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR) == -1
        assert b"smx_ctx_set_permeability" in L.smx_last_error()
        mean = np.empty((h, w), np.uint8)
        out = _lib.PairOut(mean_l=mean.ctypes.data)
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)) == -1
        assert b"mean" in L.smx_last_error()
        out = _lib.PairOut(mean_r=mean.ctypes.data)
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)) == -1
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["sgm"], None))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"semi-global" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["guided"], None))
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(smx.default_cross_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"cross-based" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_scanline(ctx, C.byref(smx.default_scanline_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1       # the chain of cross-based aggregation and the optimiser
        _lib.check(L.smx_ctx_set_cross(ctx, None))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"scan-line" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_scanline(ctx, None))
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(smx.default_cscale_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"cross-scale" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_cross_scale(ctx, None))
        _lib.check(L.smx_ctx_set_patchmatch(ctx, C.byref(smx.default_pm_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h, want_vol=False)[0] == -1 and b"permeability" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_patchmatch(ctx, None))
        rc, on = _ctx_run(ctx, (Il, Ir), None, w, h)                     # and with the conflicts gone it runs
        _lib.check(rc)
    finally:
        L.smx_destroy(ctx)
