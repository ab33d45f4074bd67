"""Cross-scale cost aggregation on the GPU (csrc/smx_cscale.hip), bit for bit against tests/cscale_ref.py:
  smx_dev_pyr_down          every border case, a width one past a workgroup's footprint, 1 / 3 / 4 channels
  smx_dev_cscale_wta_pair   random f32 volumes with ties, a NaN slice and a +inf slice -- no aggregation involved -- over shapes,
                            label ranges, 1 .. 5 scales, lambda 0 / 0.3 / 1.0, one and two views, out NULL / separate / in
                            place, the four state combinations, and level-0 volumes 0 / 4 / 8 bytes past a 16-byte boundary
                            (4, 1 and 2 pixels per lane where the width allows); every buffer in a Guarded
  the context, PairPipeline every level's aggregated volumes come from plain pipelines on the numpy pyramid (the existing
                            entries), the combination, the winners and everything behind them from the numpy references

A NaN carries no agreed payload: two values are "the same bits" here if they are both NaN or have equal bits.

Run on the GPU box:  python -m pytest tests -m gpu -q -k cscale
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import adjust_ref
import cscale_ref as ref
import subpix_ref
import uniq_ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
IDENT = np.iinfo(np.int64).max
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


def _params(scales, lam):
    p = smx.default_cscale_params()
    p.scales, p.lambda_ = scales, lam
    return p


# ---------------------------------------------------------------------------------------------
# host entries that need no device
# ---------------------------------------------------------------------------------------------
def test_defaults_weights_and_levels_equal_the_reference():
    L = smx.lib()
    p = smx.default_cscale_params()
    assert (p.scales, p.lambda_) == (4, 1.0)
    for scales, lam in itertools.product(range(1, 6), (0.0, 0.3, 1.0, 2.5, 1e-3, 1e6)):
        got = np.array(_lib.cscale_weights(_params(scales, lam)), F32)
        same(got, ref.weights(scales, lam), f"weights {scales} {lam}")
    for w, h, dmin, size_d, s in itertools.product((1, 19, 129), (1, 40), (-15, -16, -1, 0, 3), (1, 2, 16, 17), range(5)):
        assert _lib.cscale_level(w, h, dmin, size_d, s) == ref.level(w, h, dmin, size_d, s)
    wt = (C.c_float * 5)()
    for bad in (_params(0, 1.0), _params(6, 1.0), _params(2, -0.1), _params(2, float("nan")), _params(2, float("inf"))):
        assert L.smx_cscale_weights(C.byref(bad), wt) == -1 and b"scales" in L.smx_last_error()


# ---------------------------------------------------------------------------------------------
# the pyramid
# ---------------------------------------------------------------------------------------------
def _footprint():
    cols, rows = C.c_int(), C.c_int()
    _lib.check(smx.lib().smx_pyr_down_geometry(C.byref(cols), C.byref(rows)))
    return cols.value, rows.value


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_pyr_down(ch):
    cols, rows = _footprint()
    shapes = [(1, 1), (2, 1), (1, 2), (5, 3), (19, 40), (129, 70), (2 * cols + 1, 2 * rows + 1), (cols + 1, 3)]
    L = smx.lib()
    for i, (w, h) in enumerate(shapes):
        img = np.random.default_rng(100 * ch + i).integers(0, 256, (h, w, ch)).astype(np.uint8)
        img[h // 2:, : w // 2] = 255                       # (saturated: the rounding must not wrap)
        want = ref.pyr_down(img)
        src = Guarded(img.nbytes, np.uint8, img.shape, plane=w * h).load(img)
        dst = Guarded(want.nbytes, np.uint8, want.shape, plane=w * h)
        _lib.check(L.smx_dev_pyr_down(src.ptr, dst.ptr, w, h, ch, _stream()))
        dst.check(f"{w} x {h} x {ch} dst")
        src.check_unchanged(f"{w} x {h} x {ch} src")
        same(dst.numpy(), want, f"{w} x {h} x {ch}")
        same(smx.pyr_down(img if ch > 1 else img[:, :, 0]), want if ch > 1 else want[:, :, 0], f"host entry {w} x {h} x {ch}")


def test_pyr_down_refusals():
    L = smx.lib()
    g = Guarded(64, np.uint8, (64,))
    for args in ((g.ptr, g.ptr, 4, 4, 2), (g.ptr, g.ptr, 0, 4, 1), (g.ptr, g.ptr, 4, 0, 1), (None, g.ptr, 4, 4, 1),
                 (g.ptr, None, 4, 4, 1), (g.ptr, g.ptr, 1 << 16, 1 << 15, 1)):
        assert L.smx_dev_pyr_down(*args, _stream()) == -1
    g.check_untouched("refused calls")


# ---------------------------------------------------------------------------------------------
# the combination and its winner-take-all pass on random volumes
# ---------------------------------------------------------------------------------------------
def _volumes(rng, w, h, dmin, size_d, scales):
    """levels of one view: level 0 from a small set of values (ties), a NaN slice and a +inf slice where there are three slices,
    else on half the pixels; a few NaN, inf and -0 cells in every level"""
    out = []
    for s in range(scales):
        ws, hs, _, ds = ref.level(w, h, dmin, size_d, s)
        v = (rng.integers(-3, 4, (ds, hs, ws)) * 0.5).astype(F32) if s == 0 else rng.standard_normal((ds, hs, ws)).astype(F32)
        flat = v.reshape(-1)
        for val in (np.nan, np.inf, -np.inf, -0.0):
            flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = val
        out.append(v)
    a, b = (int(rng.integers(0, size_d)), int(rng.integers(0, size_d)))
    if size_d >= 3:
        b = b if b != a else (a + 1) % size_d
        out[0][a] = np.nan
        out[0][b] = np.inf
    else:
        out[0][a, :, : (w + 1) // 2] = np.nan
        out[0][b, : (h + 1) // 2, w // 2:] = np.inf
    return out


def _want_view(levels, dmin, size_d, lam):
    out = ref.combine(levels, dmin, size_d, lam)
    z, c0, lo, hi, last = subpix_ref.winners(out)
    _, _, sec, rest, last_u, _ = uniq_ref.second_best(out)
    return dict(out=out, keys=ref.pack_keys(z, c0), nbr=np.stack([lo, hi, last]).astype(F32),
                uq=np.stack([sec, rest, last_u]).astype(F32))


FORMS = list(itertools.product(("both", "left", "right"), ("none", "separate", "in place"), (False, True), (False, True)))


def _call(levels, wants, w, h, dmins, size_d, p, views, store, nbr, uq, misalign):
    """one smx_dev_cscale_wta_pair on guarded buffers; checks everything it wrote and everything it must not write"""
    L = smx.lib()
    n = w * h
    used = [0, 1] if views == "both" else [0] if views == "left" else [1]
    V = len(used)
    name = f"{w}x{h} dmin {dmins} D {size_d} scales {p.scales} lambda {p.lambda_} {views} out {store} nbr {nbr} uq {uq} +{misalign}B"
    # level 0 of the given views in one buffer, laid out as the outputs are: in place, d_out is this buffer
    lv0 = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), misalign=misalign, plane=n)
    lv0.load(np.stack([levels[v][0] for v in used]))
    coarse = [[Guarded(levels[v][s].nbytes, F32, levels[v][s].shape, misalign=4 * (s % 2), plane=n).load(levels[v][s])
               for s in range(1, p.scales)] for v in used]
    arrays = [None, None]
    for k, v in enumerate(used):
        ptrs = [lv0.ptr.value + k * size_d * n * 4] + [g.ptr.value for g in coarse[k]]
        arrays[v] = (C.c_void_p * p.scales)(*ptrs)
    keys = Guarded(V * n * 8, np.int64, (V, h, w), plane=n, fill=0x11)
    out = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), misalign=misalign, plane=n) if store == "separate" else None
    gn = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if nbr else None
    gu = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if uq else None
    d_out = lv0.ptr if store == "in place" else out.ptr if out else None
    _lib.check(L.smx_dev_cscale_wta_pair(C.byref(p), arrays[0], arrays[1], w, h, dmins[0], dmins[1], size_d, keys.ptr, d_out,
                                         gn.ptr if gn else None, gu.ptr if gu else None, _stream()))
    for k, g in enumerate(coarse):
        for s, c in enumerate(g):
            c.check_unchanged(f"{name}: level {s + 1} of view {used[k]}")
    if store == "in place":
        lv0.check(name + ": level 0 / out")
    else:
        lv0.check_unchanged(name + ": level 0")
    got_out = lv0.numpy() if store == "in place" else out.numpy() if out else None
    for g, what in ((keys, "keys"), (out, "out"), (gn, "nbr"), (gu, "uq")):
        if g is not None:
            g.check(f"{name}: {what}")
    for k, v in enumerate(used):
        same(keys.numpy()[k], wants[v]["keys"], f"{name}: keys of view {v}")
        if got_out is not None:
            same(got_out[k], wants[v]["out"], f"{name}: out of view {v}")
        if gn:
            same(gn.numpy()[k], wants[v]["nbr"], f"{name}: nbr of view {v}")
        if gu:
            same(gu.numpy()[k], wants[v]["uq"], f"{name}: uq of view {v}")


@pytest.mark.parametrize("dmin,size_d", [(-15, 16), (-16, 17), (3, 1), (-1, 2)])
# (the issue's shapes, and two whose width lets a lane take four pixels: one inside a workgroup's 512 x 2 pixels, one past them)
@pytest.mark.parametrize("w,h", [(2, 1), (19, 40), (129, 70), (20, 9), (516, 3)])
def test_combine_and_winners(w, h, dmin, size_d):
    rng = np.random.default_rng(w * 1000 + h * 10 + size_d)
    dmins = (dmin, dmin + 5)                       # (the right view's ancestors fall on other boundaries)
    levels = [_volumes(rng, w, h, d, size_d, 5) for d in dmins]
    forms = itertools.cycle(FORMS)
    k = 0
    for scales, lam in itertools.product(range(1, 6), (0.0, 0.3, 1.0)):
        wants = [_want_view(levels[v][:scales], dmins[v], size_d, lam) for v in range(2)]
        if scales == 1:
            for v in range(2):                      # out is A_0 itself, the keys the plain pass's
                same(wants[v]["out"], levels[v][0], "one scale returns level 0")
        for _ in range(5):                          # 75 calls: every form about twice, at changing scales and lambda
            views, store, nbr, uq = next(forms)
            _call(levels, wants, w, h, dmins, size_d, _params(scales, lam), views, store, nbr, uq, (0, 4, 8)[k % 3])
            k += 1


def test_one_scale_keeps_the_plain_keys():
    """scales 1: out is A_0 bit for bit and the keys are those of the plain winner-take-all rule on the same volume -- the
    rule every aggregation's pass is held to (subpix_ref.winners in tests/test_gpu_wta_pass.py)"""
    import oracle
    w, h, size_d, dmin = 154, 6, 17, -16
    Il, Ir = synth.gen_pair(w, h, size_d, 1546)
    vol = oracle.stereo_pair(Il, Ir, size_d, dminl=dmin, dminr=2, want_agg=True)["aggl"]
    z, c0 = subpix_ref.winners(vol)[:2]
    want = dict(out=vol, keys=np.where(z >= 0, oracle.pack_keys(c0, np.maximum(z, 0)), IDENT))
    # the library's own natural-order winner-take-all pass (wta_launch) over the same volume, on guarded buffers
    L = smx.lib()
    L.smx_debug_wta_natural.restype = C.c_int
    L.smx_debug_wta_natural.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    q = Guarded(vol.nbytes, F32, vol.shape, plane=w * h).load(vol)
    plain = Guarded(w * h * 8, np.int64, (h, w), plane=w * h, fill=0x11)
    _lib.check(L.smx_debug_wta_natural(q.ptr, w, h, size_d, plain.ptr, _stream()))
    plain.check("wta_launch keys")
    q.check_unchanged("wta_launch volume")
    same(plain.numpy(), want["keys"], "wta_launch against the numpy rule")
    for lam in (0.0, 1.0):
        p = _params(1, lam)
        ptrs = (C.c_void_p * 1)(q.ptr.value)
        keys = Guarded(w * h * 8, np.int64, (h, w), plane=w * h, fill=0x22)
        _lib.check(L.smx_dev_cscale_wta_pair(C.byref(p), ptrs, None, w, h, dmin, 0, size_d, keys.ptr, None, None, None, _stream()))
        keys.check("one-scale keys")
        same(keys.numpy(), plain.numpy(), f"one scale, lambda {lam}: keys against wta_launch's")
        _call([[vol]], [want], w, h, (dmin, 0), size_d, _params(1, lam), "left", "separate", False, False, 0)
        out, best, disp = smx.cross_scale_combine([vol], dmin, _params(1, lam))
        same(out, vol, "host entry out")
        same(disp, ref.label_map(z, dmin), "host entry labels")
        same(best, c0, "host entry best")


def test_combine_refusals():
    L = smx.lib()
    g = Guarded(4096, F32, (1024,))
    one = (C.c_void_p * 5)(*([g.ptr.value] * 5))
    odd = (C.c_void_p * 5)(*([g.ptr.value + 2] * 5))
    null = (C.c_void_p * 5)(g.ptr.value, 0, 0, 0, 0)
    ok = _params(2, 1.0)
    calls = [(_params(0, 1.0), one, None, 4, 4, 0, 0, 2), (_params(6, 1.0), one, None, 4, 4, 0, 0, 2),
             (_params(2, -1.0), one, None, 4, 4, 0, 0, 2), (_params(2, float("nan")), one, None, 4, 4, 0, 0, 2),
             (ok, None, None, 4, 4, 0, 0, 2), (ok, one, None, 0, 4, 0, 0, 2), (ok, one, None, 4, 4, 0, 0, 0),
             (ok, one, None, 1 << 16, 1 << 15, 0, 0, 2), (ok, odd, None, 4, 4, 0, 0, 2), (ok, null, None, 4, 4, 0, 0, 2),
             (ok, None, null, 4, 4, 0, 0, 2), (ok, one, None, 4, 4, 1 << 30, 0, 2)]
    for c in calls:
        assert L.smx_dev_cscale_wta_pair(C.byref(c[0]), *c[1:], g.ptr, None, None, None, _stream()) == -1, c
        assert L.smx_last_error()
    assert L.smx_dev_cscale_wta_pair(C.byref(ok), one, None, 4, 4, 0, 0, 2, None, None, None, None, _stream()) == -1
    g.check_untouched("refused calls")


# ---------------------------------------------------------------------------------------------
# the context and PairPipeline
# ---------------------------------------------------------------------------------------------
D, DMINL, DMINR = 16, -15, 0


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
    p.colour = 1
    return p


def _pipe_kw(cost, guide):
    """cost "adcensus": AD-Census with its absolute differences on the colour images"""
    kw = dict(cost=None if cost == "reference" else cost, guidance="rgb" if guide == "rgb" else None)
    if cost == "adcensus":
        kw["adcensus_params"] = _adc()
    return kw


def _level_volumes(gray, rgb, w, h, cost, guide, scales):
    """every level's aggregated volumes of both views through plain pipelines (no cross-scale) on the numpy pyramid"""
    from stereo_matching_cuda_amd.device import PairPipeline
    pg = [ref.pyramid(g, scales) for g in gray]
    pc = [ref.pyramid(c, scales) for c in rgb] if rgb else None
    levels = ([], [])
    for s in range(scales):
        ws, hs, dl, sl = ref.level(w, h, DMINL, D, s)
        _, _, dr, sr = ref.level(w, h, DMINR, D, s)
        pipe = PairPipeline(ws, hs, max(sl, sr), dminl=dl, dminr=dr, want_agg=True, **_pipe_kw(cost, guide))
        kw = dict(rgb_l=_t(pc[0][s]), rgb_r=_t(pc[1][s])) if rgb else {}
        pipe.run(_t(pg[0][s]), _t(pg[1][s]), **kw)
        r = pipe.results()
        levels[0].append(r["aggl"][:sl].copy())
        levels[1].append(r["aggr"][:sr].copy())
    return levels


def _want_pair(orc, levels, lam, chain=None):
    """the pair's outputs from the levels' volumes through the numpy references; chain: dict(mode, ratio, adjust) or None"""
    comb = [ref.combine(levels[v], (DMINL, DMINR)[v], D, lam) for v in range(2)]
    win = [subpix_ref.winners(c) for c in comb]
    r = {"aggl": comb[0], "aggr": comb[1]}
    for v, side in enumerate("lr"):
        z, c0 = win[v][:2]
        took = (z >= 0) & (PRESET >= c0)
        r["dmap" + side] = subpix_ref.dmap_of(z, c0, (DMINL, DMINR)[v])
        r["best" + side] = np.where(took, c0, PRESET).astype(F32)
    r["occlusion"] = orc.detect_occlusion(r["dmapl"], r["dmapr"], DMINL - 100)
    r["filled"] = orc.fill_occlusion(r["occlusion"], DMINL)
    if chain:
        z, c0, lo, hi, _ = win[0]
        sec = uniq_ref.second_best(comb[0])[2]
        r["unique"], r["margin"] = uniq_ref.apply(r["occlusion"], z >= 0, c0, sec, chain["ratio"], DMINL, DMINL - 100)
        filled = orc.fill_occlusion(r["unique"], DMINL)
        r["subpixl"], sub_filled = subpix_ref.maps(chain["mode"], z, c0, lo, hi, r["dmapl"], r["unique"], filled, DMINL)
        zr, cr, lor, hir, _ = win[1]
        r["subpixr"] = subpix_ref.maps(chain["mode"], zr, cr, lor, hir, r["dmapr"])[0]
        r["adjusted"], r["subpix_filled"] = adjust_ref.adjust(filled, comb[0], DMINL, mode=chain["mode"], sub=sub_filled,
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
@pytest.mark.parametrize("cost", ["reference", "census"])
@pytest.mark.parametrize("w,h,scales,lam", [(19, 40, 3, 0.3), (129, 70, 4, 1.0)])
def test_context_and_pipeline(orc, w, h, scales, lam, cost, guide):
    from stereo_matching_cuda_amd.device import PairPipeline
    L = smx.lib()
    gray, rgb = _images(w, h, guide, 7 * w + scales)
    levels = _level_volumes(gray, rgb, w, h, cost, guide, scales)
    want = _want_pair(orc, levels, lam)
    kw = dict(rgb_l=_t(rgb[0]), rgb_r=_t(rgb[1])) if rgb else {}
    name = f"{w}x{h} {cost} {guide}"
    # PairPipeline
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, cross_scale=_params(scales, lam), **_pipe_kw(cost, guide))
    pipe.run(_t(gray[0]), _t(gray[1]), **kw)
    got = pipe.results()
    for _, k in CTX_NAMES:
        same(got[k], want[k], f"{name} pipeline {k}")
    # ... and one scale is the plain pipeline
    plain = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, want_agg=True, **_pipe_kw(cost, guide))
    plain.run(_t(gray[0]), _t(gray[1]), **kw)
    one = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, cross_scale=_params(1, lam), **_pipe_kw(cost, guide))
    one.run(_t(gray[0]), _t(gray[1]), **kw)
    a, b = plain.results(), one.results()
    assert sorted(a) == sorted(b)
    for k in a:
        same(b[k], a[k], f"{name} one scale, pipeline {k}")
    same(one.keys.cpu().numpy(), plain.keys.cpu().numpy(), f"{name} one scale, pipeline keys")
    # the context: off, on, one scale, off again
    ctx = _ctx(w, h, cost, guide)
    try:
        rc, off = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(scales, lam))))
        for want_vol in (True, False):
            rc, on = _ctx_run(ctx, gray, rgb, w, h, want_vol)
            _lib.check(rc)
            for k, n in CTX_NAMES[:8 if want_vol else 6]:
                same(on[k], want[n], f"{name} context {k}")
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(1, lam))))
        rc, single = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_cross_scale(ctx, None))
        rc, again = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        for k, _ in CTX_NAMES:
            same(single[k], off[k], f"{name} context, one scale {k}")
            same(again[k], off[k], f"{name} context, off again {k}")
    finally:
        L.smx_destroy(ctx)


@pytest.mark.parametrize("guide", ["gray", "rgb"])
def test_adcensus_reads_the_colour_pyramid(orc, guide):
    """AD-Census with colour 1: a level's absolute differences come from the level of the colour pyramid, its census codes from
    the level of the gray pyramid (not from the gray of the level's colour image)"""
    from stereo_matching_cuda_amd.device import PairPipeline
    w, h, scales, lam = 129, 70, 3, 1.0
    gray, rgb = _images(w, h, "rgb", 23)
    want = _want_pair(orc, _level_volumes(gray, rgb, w, h, "adcensus", guide, scales), lam)
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, cross_scale=_params(scales, lam), **_pipe_kw("adcensus", guide))
    pipe.run(_t(gray[0]), _t(gray[1]), rgb_l=_t(rgb[0]), rgb_r=_t(rgb[1]))
    got = pipe.results()
    for _, k in CTX_NAMES:
        same(got[k], want[k], f"adcensus {guide} pipeline {k}")
    ctx = _ctx(w, h, "adcensus", guide)
    try:
        _lib.check(smx.lib().smx_ctx_set_cross_scale(ctx, C.byref(_params(scales, lam))))
        rc, on = _ctx_run(ctx, gray, rgb, w, h)
        _lib.check(rc)
        for k, n in CTX_NAMES:
            same(on[k], want[n], f"adcensus {guide} context {k}")
    finally:
        smx.lib().smx_destroy(ctx)


def test_coarsest_level_of_two_columns(orc):
    """19 x 40 at five scales: level 4 is 2 x 3, the narrowest a context takes"""
    from stereo_matching_cuda_amd.device import PairPipeline
    w, h, scales, lam = 19, 40, 5, 1.0
    gray, _ = _images(w, h, "gray", 3)
    want = _want_pair(orc, _level_volumes(gray, None, w, h, "reference", "gray", scales), lam)
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, cross_scale=_params(scales, lam))
    pipe.run(_t(gray[0]), _t(gray[1]))
    got = pipe.results()
    for _, k in CTX_NAMES:
        same(got[k], want[k], f"pipeline {k}")
    ctx = _ctx(w, h, "reference", "gray")
    try:
        _lib.check(smx.lib().smx_ctx_set_cross_scale(ctx, C.byref(_params(scales, lam))))
        rc, on = _ctx_run(ctx, gray, None, w, h)
        _lib.check(rc)
        for k, n in CTX_NAMES:
            same(on[k], want[n], f"context {k}")
    finally:
        smx.lib().smx_destroy(ctx)


@pytest.mark.parametrize("mode", ["parabola", "equiangular"])
def test_the_stages_behind_run_on_the_combined_volume(orc, mode):
    """sub-pixel + uniqueness + adjustment on: every output is the chain of the existing numpy references on the combined
    volumes"""
    from stereo_matching_cuda_amd.device import PairPipeline
    L = smx.lib()
    w, h, scales, lam, ratio = 129, 70, 3, 1.0, 0.05
    adj = dict(tau_e=2, vertical=1, iterations=2)
    gray, _ = _images(w, h, "gray", 11)
    levels = _level_volumes(gray, None, w, h, "reference", "gray", scales)
    want = _want_pair(orc, levels, lam, dict(mode=subpix_ref.MODES[mode], ratio=ratio, adjust=adj))
    ap = smx.default_adjust_params()
    ap.tau_e, ap.vertical, ap.iterations = adj["tau_e"], adj["vertical"], adj["iterations"]
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, cross_scale=_params(scales, lam), subpixel=mode, uniqueness=ratio,
                        adjust=ap)
    pipe.run(_t(gray[0]), _t(gray[1]))
    got = pipe.results()
    for k in ("bestl", "bestr", "dmapl", "dmapr", "occlusion", "unique", "margin", "filled", "adjusted", "subpixl", "subpixr",
              "subpix_filled", "aggl", "aggr"):
        same(got[k], want[k], f"pipeline {k}")
    ctx = _ctx(w, h, "reference", "gray")
    try:
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(scales, lam))))
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
    levels, nbytes = C.c_int(-1), C.c_size_t(1)
    _lib.check(smx.lib().smx_ctx_cscale_held(ctx, C.byref(levels), C.byref(nbytes)))
    return levels.value, nbytes.value


def test_a_context_without_the_setter_allocates_nothing_new():
    """Off by default: a context whose pairs never ran with cross-scale on holds no level and no byte for it -- whether the
    setter was never called, or called and switched off again before the first pair (smx_ctx_cscale_held counts the levels'
    contexts and every device buffer of theirs: nothing else of the feature allocates).  Once a pair ran with it on, the levels stay until smx_destroy (include/smx.h)."""
    import torch
    L = smx.lib()
    w, h = 129, 70
    (Il, Ir), _ = _images(w, h, "gray", 5)

    def used_by(prepare):
        """device bytes a context takes from create to after its first pair, as the driver counts them"""
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        ctx = _ctx(w, h, "reference", "gray")
        try:
            prepare(ctx)
            _lib.check(_ctx_run(ctx, (Il, Ir), None, w, h, want_vol=False)[0])
            return before - torch.cuda.mem_get_info()[0], _held(ctx)
        finally:
            L.smx_destroy(ctx)

    def set_and_unset(ctx):
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(4, 1.0))))
        _lib.check(L.smx_ctx_set_cross_scale(ctx, None))

    used_by(lambda ctx: None)                                   # (warms the driver's pools)
    never, held_never = used_by(lambda ctx: None)
    unset, held_unset = used_by(set_and_unset)
    on, held_on = used_by(lambda ctx: _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(4, 1.0)))))
    print("device bytes of a context and its first pair: never set", never, "set and unset", unset, "on", on, held_on)
    assert held_never == (0, 0) and held_unset == (0, 0)
    assert held_on[0] == 3 and held_on[1] > 0
    # (the driver's figures are printed, not asserted: the card may serve other processes, whose allocations move them)
    ctx = _ctx(w, h, "reference", "gray")
    try:
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(3, 1.0))))
        _lib.check(_ctx_run(ctx, (Il, Ir), None, w, h, want_vol=False)[0])
        assert _held(ctx)[0] == 2
        _lib.check(L.smx_ctx_set_cross_scale(ctx, None))
        _lib.check(_ctx_run(ctx, (Il, Ir), None, w, h, want_vol=False)[0])
        assert _held(ctx)[0] == 2                               # kept for the next time
    finally:
        L.smx_destroy(ctx)


def test_refused_combinations():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    L = smx.lib()
    w, h = 40, 19
    for agg in ("sgm", "cross", "scanline", "cross-scanline"):
        with pytest.raises(ValueError):
            PairPipeline(w, h, D, cross_scale=True, aggregation=agg)
    for bad in (dict(s_begin=1), dict(s_end=D - 1), dict(cross_scale=_params(0, 1.0)), dict(cross_scale=_params(6, 1.0)),
                dict(cross_scale=_params(2, -1.0)), dict(cross_scale=4)):
        with pytest.raises(ValueError):
            PairPipeline(w, h, D, **{"cross_scale": True, **bad})
    with pytest.raises(ValueError):
        PairPipeline(5, 8, D, cross_scale=_params(4, 1.0))              # level 3 is one column wide
    with pytest.raises(ValueError):
        ShardedPair(w, h, D, cross_scale=True)
    pipe = PairPipeline(w, h, D, cross_scale=_params(2, 1.0))
    (Il, Ir), _ = _images(w, h, "gray", 1)
    with pytest.raises(ValueError):
        pipe.aggregate(_t(Il), _t(Ir), _t(np.zeros((D, h, w), F32)), _t(np.zeros((D, h, w), F32)))
    ctx = _ctx(w, h, "reference", "gray")
    try:
        for bad in (_params(0, 1.0), _params(6, 1.0), _params(2, -1.0), _params(2, float("inf"))):
            assert L.smx_ctx_set_cross_scale(ctx, C.byref(bad)) == -1 and b"scales" in L.smx_last_error()
        rc, plain = _ctx_run(ctx, (Il, Ir), None, w, h)                 # a refused setter leaves it off
        _lib.check(rc)
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(2, 1.0))))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR) == -1
        assert b"smx_ctx_set_cross_scale" in L.smx_last_error()
        mean = np.empty((h, w), np.uint8)
        out = _lib.PairOut(mean_l=mean.ctypes.data)
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)) == -1
        assert b"mean" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["sgm"], None))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"semi-global" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["guided"], None))
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(smx.default_cross_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"cross-based" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_cross(ctx, None))
        _lib.check(L.smx_ctx_set_scanline(ctx, C.byref(smx.default_scanline_params())))
        assert _ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"scan-line" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_scanline(ctx, None))
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(_params(5, 1.0))))    # 40 x 19: level 4 is 3 x 2 -- fine
        _lib.check(_ctx_run(ctx, (Il, Ir), None, w, h)[0])
    finally:
        L.smx_destroy(ctx)
    small = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), 5, 8, D, C.byref(small)))
    try:
        _lib.check(L.smx_ctx_set_cross_scale(small, C.byref(_params(4, 1.0))))
        (Sl, Sr), _ = _images(5, 8, "gray", 2)
        assert _ctx_run(small, (Sl, Sr), None, 5, 8)[0] == -1 and b"narrower" in L.smx_last_error()
    finally:
        L.smx_destroy(small)
