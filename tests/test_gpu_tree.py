"""The non-local tree filter on the GPU (csrc/smx_tree.hip), bit for bit against tests/tree_ref.py:
  smx_dev_tree_wta_pair  random f32 volumes with ties, -0 and, in one slice each, a NaN and an infinity -- no aggregation
                         involved -- over the shapes below, 1 / 3 / 4 channels, one and two views, out NULL / separate / in
                         place, d_keys NULL, the four state combinations, one chunk of slices against several; every buffer in a
                         Guarded, the workspace poisoned with NaN bits
  smx_tree_filter        the host entry, through stages.tree_filter, and device.tree_filter_pair
  the context            the aggregated volumes come from the oracle (reference cost, gray guide) or from a plain pipeline
                         (colour guide), the filter, the winners and everything behind them from the numpy references

The shapes are the smallest that can still go wrong.  1 x 1: one node, no level loop.  64 x 1 and 1 x 64: a path, levels == n,
the deepest tree there is: the most barriers on the fewest nodes.  2 x 2.  A constant 300 x 300: the comb, whose widest level
holds 300 nodes, more than the 256 threads of the workgroup (the stride loop).  65 x 9 and 129 x 70 with 18 slices: several
workgroups a view, levels of every width.  There is no LDS-staged size limit and no vector width: every access is a 4-byte one.

A NaN carries no agreed payload: two values are "the same bits" here if they are both NaN or have equal bits.

Run on the GPU box:  python -m pytest tests -m gpu -q -k tree
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import adjust_ref
import subpix_ref
import test_gpu_perm as tp
import tree_ref as ref
import uniq_ref
from guarded import SMX_E_WS, Guarded
from test_gpu_perm import same

pytestmark = pytest.mark.gpu

F32 = np.float32
PRESET = np.uint32(0x7F7F7F7F).view(F32)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _params(sigma):
    p = smx.default_tree_params()
    p.sigma = sigma
    return p


def _volume(rng, w, h, size_d, smooth):
    """a view's volume: few distinct values (ties) or normal ones, -0 in many places.  A NaN or an infinity reaches every pixel
    of its slice along the tree and no other slice: with three slices or more one slice gets a NaN and another a +inf."""
    v = (rng.integers(-3, 4, (size_d, h, w)) * 0.5).astype(F32) if smooth else rng.standard_normal((size_d, h, w)).astype(F32)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, max(1, flat.size // 97))] = -0.0
    if size_d >= 3:
        for z, val in zip(rng.permutation(size_d), (np.nan, np.inf)):
            v[z, rng.integers(0, h), rng.integers(0, w)] = val
    return v


def _guide(rng, w, h, ch, kind):
    if kind == "random":
        g = rng.integers(0, 256, (h, w, ch))
    elif kind == "patches":                    # flat patches with a few edges, +-2 of noise: many ties among the small weights
        base = rng.integers(0, 256, (h // 7 + 1, w // 5 + 1, ch)).astype(np.int64)
        g = np.clip(np.kron(base, np.ones((7, 5, 1), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w, ch)), 0, 255)
    elif kind == "two":
        g = rng.integers(0, 2, (h, w, ch)) * 9 + 100
    elif kind == "extreme":
        g = rng.integers(0, 2, (h, w, ch)) * 255
    else:
        g = np.full((h, w, ch), 131)
    g = g.astype(np.uint8)
    return np.ascontiguousarray(g[:, :, 0] if ch == 1 else g)


def _want_view(vol, tree, guide, sigma):
    out = ref.filter_volume(vol, guide, sigma, tree)
    z, c0, lo, hi, last = subpix_ref.winners(out)
    _, _, sec, rest, last_u, _ = uniq_ref.second_best(out)
    return dict(out=out, keys=ref.pack_keys(z, c0), nbr=np.stack([lo, hi, last]).astype(F32),
                uq=np.stack([sec, rest, last_u]).astype(F32))


class Case:
    """two views' volumes, guides, trees and -- computed once, shared by every call on the case -- what a call must give"""

    def __init__(self, seed, w, h, size_d, ch, kind, sigma):
        rng = np.random.default_rng(seed)
        self.w, self.h, self.size_d, self.ch, self.sigma = w, h, size_d, ch, sigma
        self.vols = [_volume(rng, w, h, size_d, smooth=v == 0) for v in range(2)]
        self.guides = [_guide(rng, w, h, ch, kind) for _ in range(2)]
        self.trees = [ref.build(g) for g in self.guides]
        self.blobs = [ref.blob(t) for t in self.trees]
        self.wants = [_want_view(self.vols[v], self.trees[v], self.guides[v], sigma) for v in range(2)]
        self.name = f"{w}x{h} D {size_d} ch {ch} {kind} sigma {sigma} levels {[t['levels'] for t in self.trees]}"


FORMS = list(itertools.product(("both", "left", "right"), ("none", "separate", "in place"), (False, True), (False, True)))


def _call(c, views, store, nbr, uq, ws_slices=None, expect=0, with_keys=True):
    """one smx_dev_tree_wta_pair on guarded buffers; checks everything it wrote and everything it must not write.  ws_slices: the
    slices in flight the workspace is sized for (None: all of them, 0: four bytes short of one); expect: the return code"""
    L = smx.lib()
    w, h, size_d = c.w, c.h, c.size_d
    n = w * h
    used = [0, 1] if views == "both" else [0] if views == "left" else [1]
    V = len(used)
    name = f"{c.name} {views} out {store} keys {with_keys} nbr {nbr} uq {uq} ws for {ws_slices}"
    vin = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), plane=n).load(np.stack([c.vols[v] for v in used]))
    td = [Guarded(c.blobs[v].nbytes, np.uint8, c.blobs[v].shape, plane=n).load(c.blobs[v]) for v in used]
    keys = Guarded(V * n * 8, np.int64, (V, h, w), plane=n, fill=0x11) if with_keys else None
    out = Guarded(V * size_d * n * 4, F32, (V, size_d, h, w), plane=n) if store == "separate" else None
    gn = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if nbr else None
    gu = Guarded(V * 3 * n * 4, F32, (V, 3, h, w), plane=n) if uq else None
    per = V * n * 4 * (2 if store == "none" else 1)
    k = size_d if ws_slices is None else ws_slices
    ws_bytes = per * k if k else per - 4
    ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), plane=n, fill=0xFF)
    ptrs = [None, None], [None, None]
    for i, v in enumerate(used):
        ptrs[0][v] = C.c_void_p(vin.ptr.value + i * size_d * n * 4)
        ptrs[1][v] = td[i].ptr
    d_out = vin.ptr if store == "in place" else out.ptr if out else None
    rc = L.smx_dev_tree_wta_pair(C.byref(_params(c.sigma)), ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1], w, h, -3, 2, size_d,
                                 keys.ptr if keys else None, d_out, gn.ptr if gn else None, gu.ptr if gu else None, ws.ptr, ws_bytes,
                                 _stream())
    assert rc == expect, (name, rc, L.smx_last_error())
    for g in td:
        g.check_unchanged(name + ": tree")
    guards = ((keys, "keys"), (out, "out"), (gn, "nbr"), (gu, "uq"), (ws, "workspace"))
    if rc != 0:
        vin.check_unchanged(name + ": volume of a refused call")
        for g, what in guards:
            if g is not None:
                g.check_untouched(f"{name}: {what} of a refused call")
        return None
    if store == "in place":
        vin.check(name + ": volume / out")
    else:
        vin.check_unchanged(name + ": volume")
    got_out = vin.numpy() if store == "in place" else out.numpy() if out else None
    for g, what in guards:
        if g is not None:
            g.check(f"{name}: {what}")
    for i, v in enumerate(used):
        if keys:
            same(keys.numpy()[i], c.wants[v]["keys"], f"{name}: keys of view {v}")
        if got_out is not None:
            same(got_out[i], c.wants[v]["out"], f"{name}: out of view {v}")
        if gn:
            same(gn.numpy()[i], c.wants[v]["nbr"], f"{name}: nbr of view {v}")
        if gu:
            same(gu.numpy()[i], c.wants[v]["uq"], f"{name}: uq of view {v}")
    return dict(keys=keys.numpy() if keys else None, out=got_out, nbr=gn.numpy() if gn else None, uq=gu.numpy() if gu else None)


# (w, h, slices, channels, guide): the shapes of the module's docstring with random, two-valued, extreme and constant guides
SHAPES = [(1, 1, 3, 1, "random"), (64, 1, 3, 1, "random"), (1, 64, 3, 3, "two"), (2, 2, 4, 4, "random"), (300, 300, 2, 1, "constant"),
          (65, 9, 18, 1, "patches"), (65, 9, 18, 3, "extreme"), (129, 70, 18, 1, "random"), (129, 70, 18, 4, "two"),
          (129, 70, 18, 3, "patches")]


@pytest.mark.parametrize("w,h,size_d,ch,kind", SHAPES)
def test_filter_and_winners(w, h, size_d, ch, kind):
    at = SHAPES.index((w, h, size_d, ch, kind))
    c = Case(w * 1000 + h + ch, w, h, size_d, ch, kind, (25.5, 4.0, 0.011, 200.0)[at % 4])
    if size_d >= 3:          # (the NaN's and the infinity's slices are lost whole, every other slice is untouched by them)
        for v in range(2):
            hit = ~np.isfinite(c.wants[v]["out"]).reshape(size_d, -1)
            assert (hit.all(axis=1) | ~hit.any(axis=1)).all() and hit.all(axis=1).sum() == 2
    forms = itertools.cycle(FORMS[(7 * at) % len(FORMS):] + FORMS)
    for _ in range(6):
        _call(c, *next(forms))
    if kind == "constant":   # the comb: w + h - 1 levels, the widest of min(w, h) nodes: more than the workgroup has threads
        assert c.trees[0]["levels"] == w + h - 1 and int(np.diff(c.trees[0]["level_start"].astype(np.int64)).max()) == min(w, h) > 256


def test_every_form_on_one_shape():
    """all 36 combinations of views, output and states on 65 x 9 x 3, and the calls without keys"""
    c = Case(5, 65, 9, 3, 3, "patches", 25.5)
    for form in FORMS:
        _call(c, *form)
    for views, store in (("both", "separate"), ("left", "in place"), ("right", "separate")):
        _call(c, views, store, False, False, with_keys=False)


@pytest.mark.parametrize("store", ["none", "separate", "in place"])
def test_chunks_of_slices_give_the_same_bits(store):
    """a workspace for all 18 slices in flight (one chunk) against ones for 5, 2 and exactly 1, and the calling thread's
    smx_set_max_slices_per_launch"""
    L = smx.lib()
    c = Case(17, 70, 33, 18, 1, "patches", 25.5)
    whole = _call(c, "both", store, True, True)
    for k in (5, 2, 1):
        part = _call(c, "both", store, True, True, ws_slices=k)
        for name in whole:
            if whole[name] is not None:
                same(part[name], whole[name], f"{store}, {k} slices in flight: {name}")
    _lib.check(L.smx_set_max_slices_per_launch(3))
    try:
        _call(c, "left", store, True, False)
        _call(c, "both", store, False, True, ws_slices=7)
    finally:
        _lib.check(L.smx_set_max_slices_per_launch(0))


@pytest.mark.parametrize("views,store", [("both", "none"), ("both", "in place"), ("left", "separate"), ("right", "none")])
def test_a_workspace_below_one_slice_is_refused_before_any_launch(views, store):
    """4 bytes short of one slice in flight: SMX_E_WS, and no buffer of the call -- the poisoned workspace included -- is touched"""
    c = Case(3, 19, 40, 3, 1, "random", 25.5)
    _call(c, views, store, True, True, ws_slices=0, expect=SMX_E_WS)
    assert b"workspace" in smx.lib().smx_last_error()


def test_refused_arguments():
    L = smx.lib()
    g = Guarded(4096, F32, (1024,))
    ok = _params(25.5)
    v, odd = g.ptr, C.c_void_p(g.ptr.value + 2)
    tail = (g.ptr, None, None, None, g.ptr, 4096)
    calls = [(_params(0.0), v, None, v, None, 4, 4, 0, 0, 2), (_params(float("nan")), v, None, v, None, 4, 4, 0, 0, 2),
             (_params(float("inf")), v, None, v, None, 4, 4, 0, 0, 2), (_params(-2.0), v, None, v, None, 4, 4, 0, 0, 2),
             (ok, None, None, None, None, 4, 4, 0, 0, 2), (ok, v, None, None, None, 4, 4, 0, 0, 2), (ok, v, None, v, v, 4, 4, 0, 0, 2),
             (ok, v, None, v, None, 0, 4, 0, 0, 2), (ok, v, None, v, None, 4, 0, 0, 0, 2), (ok, v, None, v, None, 4, 4, 0, 0, 0),
             (ok, v, None, v, None, 1 << 16, 1 << 15, 0, 0, 2), (ok, odd, None, v, None, 4, 4, 0, 0, 2),
             (ok, v, None, odd, None, 4, 4, 0, 0, 2), (ok, v, None, v, None, 4, 4, 1 << 30, 0, 2)]
    for c in calls:
        assert L.smx_dev_tree_wta_pair(C.byref(c[0]), *c[1:], *tail, _stream()) == -1, c
        assert L.smx_last_error()
    # states without keys
    assert L.smx_dev_tree_wta_pair(C.byref(ok), v, None, v, None, 4, 4, 0, 0, 2, None, None, g.ptr, None, g.ptr, 4096, _stream()) == -1
    # no workspace
    assert L.smx_dev_tree_wta_pair(C.byref(ok), v, None, v, None, 4, 4, 0, 0, 2, g.ptr, None, None, None, None, 0, _stream()) == SMX_E_WS
    g.check_untouched("refused calls")


def test_host_entry_and_device_front_end(orc):
    """stages.tree_filter: an aggregated volume behind the guided filter and the paper's own form on a raw cost volume;
    device.tree_filter_pair on the same volumes"""
    import torch
    from stereo_matching_cuda_amd.device import tree_filter_pair
    w, h, size_d, dmin = 70, 20, 9, -8
    Il, Ir = synth.gen_pair(w, h, size_d, 77)
    r = orc.stereo_pair(Il, Ir, size_d, dminl=dmin, dminr=0, want_cost=True, want_agg=True)
    for vol, sigma in ((r["aggl"], None), (r["costl"], 16.0), (r["aggl"], _params(8.0))):
        s = 25.5 if sigma is None else sigma.sigma if isinstance(sigma, _lib.TreeParams) else sigma
        want = ref.filter_volume(vol, Il, s)
        z, c0 = ref.winners(want)
        out, best, disp = smx.tree_filter(vol, Il, sigma, dmin=dmin)
        same(out, want, "host entry out")
        same(best, c0, "host entry best")
        same(disp, ref.label_map(z, dmin), "host entry labels")
    rgb = np.stack([Il, Il[::-1], Il[:, ::-1]], axis=2).copy()
    same(smx.tree_filter(r["aggl"], rgb, 25.5)[0], ref.filter_volume(r["aggl"], rgb, 25.5), "host entry, colour guide")
    out_l, out_r, keys, nbr, uq = tree_filter_pair(torch.from_numpy(r["aggl"]).cuda(), torch.from_numpy(r["aggr"]).cuda(), Il, Ir,
                                                   dminl=dmin, want_states=True)
    for v, (vol, g, got) in enumerate(((r["aggl"], Il, out_l), (r["aggr"], Ir, out_r))):
        want = _want_view(vol, ref.build(g), g, 25.5)
        same(got.cpu().numpy(), want["out"], f"device front end out {v}")
        same(keys[v].cpu().numpy(), want["keys"], f"device front end keys {v}")
        same(nbr[v].cpu().numpy(), want["nbr"], f"device front end nbr {v}")
        same(uq[v].cpu().numpy(), want["uq"], f"device front end uq {v}")
    with pytest.raises(ValueError):
        smx.tree_filter(r["aggl"], Il[:-1], 25.5)


# ---------------------------------------------------------------------------------------------
# the context
# ---------------------------------------------------------------------------------------------
D, DMINL, DMINR = tp.D, tp.DMINL, tp.DMINR
W, H = tp.W, tp.H


def _want_pair(orc, vols, guides, sigma, chain=None):
    """the pair's outputs from the plain volumes through the numpy references (the chain of tests/test_gpu_perm.py with the
    tree filter in the permeability filter's place); chain: dict(mode, ratio, adjust) or None"""
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


def _held(ctx):
    nbytes = C.c_size_t(1)
    _lib.check(smx.lib().smx_ctx_tree_held(ctx, C.byref(nbytes)))
    return nbytes.value


HELD = 2 * W * H * 4 * D + 2 * ref.tree_bytes(W, H)          # the workspace of every slice of both views, and the two blobs


@pytest.mark.parametrize("entry,guide", [("gray", "gray"), ("rgb", "rgb"), ("rgb", "gray")])
def test_context(orc, entry, guide):
    """mode on against the numpy chain -- the gray entry, the colour entry under the colour guide (the trees of the colour
    images) and the colour entry under the gray guide (the trees of the device's gray images) -- and off again"""
    L = smx.lib()
    sigma = 25.5
    gray, rgb = tp._images(W, H, entry, 31)
    vols = tp._plain_volumes(orc, gray, rgb if guide == "rgb" else None, W, H, "reference", guide)
    want = _want_pair(orc, vols, rgb if guide == "rgb" else gray, sigma)
    name = f"{entry} entry, {guide} guide"
    ctx = tp._ctx(W, H, "reference", guide)
    try:
        rc, off = tp._ctx_run(ctx, gray, rgb, W, H)
        _lib.check(rc)
        assert _held(ctx) == 0
        _lib.check(L.smx_ctx_set_tree(ctx, C.byref(_params(sigma))))
        assert _held(ctx) == 0
        for want_vol in (True, False):
            rc, on = tp._ctx_run(ctx, gray, rgb, W, H, want_vol)
            _lib.check(rc)
            for k, n in tp.CTX_NAMES[:8 if want_vol else 6]:
                same(on[k], want[n], f"{name} context {k}")
        assert _held(ctx) == HELD
        _lib.check(L.smx_ctx_set_tree(ctx, None))
        rc, again = tp._ctx_run(ctx, gray, rgb, W, H)
        _lib.check(rc)
        for k, _ in tp.CTX_NAMES:
            same(again[k], off[k], f"{name} context, off again {k}")
        same(off["agg_l"], vols[0], f"{name} context, plain volume")
        assert np.count_nonzero(want["dmapl"] != off["dmap_l"]) > 0          # (the filter does change winners here)
        assert tp._held(ctx) == 0                                            # (and the permeability mode never ran)
    finally:
        L.smx_destroy(ctx)


def test_the_stages_behind_run_on_the_filtered_volume(orc):
    """sub-pixel + uniqueness + adjustment on: every output is the chain of the existing numpy references on the filtered
    volumes, the d_nbr and d_uq states of the pass included"""
    L = smx.lib()
    sigma, ratio, mode = 12.0, 0.05, "parabola"
    adj = dict(tau_e=2, vertical=1, iterations=2)
    gray, _ = tp._images(W, H, "gray", 11)
    vols = tp._plain_volumes(orc, gray, None, W, H, "reference", "gray")
    want = _want_pair(orc, vols, gray, sigma, dict(mode=subpix_ref.MODES[mode], ratio=ratio, adjust=adj))
    ap = smx.default_adjust_params()
    ap.tau_e, ap.vertical, ap.iterations = adj["tau_e"], adj["vertical"], adj["iterations"]
    ctx = tp._ctx(W, H, "reference", "gray")
    try:
        _lib.check(L.smx_ctx_set_tree(ctx, C.byref(_params(sigma))))
        _lib.check(L.smx_ctx_set_subpixel(ctx, subpix_ref.MODES[mode]))
        _lib.check(L.smx_ctx_set_uniqueness(ctx, ratio))
        _lib.check(L.smx_ctx_set_adjust(ctx, C.byref(ap)))
        rc, on = tp._ctx_run(ctx, gray, None, W, H, want_vol=False)
        _lib.check(rc)
        for k, n in tp.CTX_NAMES[:6]:
            same(on[k], want[n], f"context {k}")
        maps = [np.empty((H, W), F32) for _ in range(5)]
        _lib.check(L.smx_ctx_subpixel_maps(ctx, *[m.ctypes.data for m in maps[:3]]))
        _lib.check(L.smx_ctx_uniqueness_map(ctx, *[m.ctypes.data for m in maps[3:]]))
        for m, n in zip(maps, ("subpixl", "subpixr", "subpix_filled", "unique", "margin")):
            same(m, want[n], f"context {n}")
    finally:
        L.smx_destroy(ctx)


def test_refusals_of_the_mode():
    """the two setters refuse each other, naming both; the pipelined entry refuses; the refusals of the row under this mode's name"""
    L = smx.lib()
    w, h = 40, 19
    (Il, Ir), _ = tp._images(w, h, "gray", 1)
    perm = smx.default_perm_params()
    ctx = tp._ctx(w, h, "reference", "gray")
    try:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert L.smx_ctx_set_tree(ctx, C.byref(_params(bad))) == -1 and b"sigma" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_permeability(ctx, C.byref(perm)))
        assert L.smx_ctx_set_tree(ctx, C.byref(_params(25.5))) == -1
        assert b"smx_ctx_set_tree" in L.smx_last_error() and b"smx_ctx_set_permeability" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_tree(ctx, None))                           # (switching off is never refused)
        _lib.check(L.smx_ctx_set_permeability(ctx, None))
        _lib.check(L.smx_ctx_set_tree(ctx, C.byref(_params(25.5))))
        assert L.smx_ctx_set_permeability(ctx, C.byref(perm)) == -1
        assert b"smx_ctx_set_tree" in L.smx_last_error() and b"smx_ctx_set_permeability" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_tree(ctx, C.byref(_params(9.0))))          # (its own mode again: new parameters)
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR) == -1
        assert b"smx_ctx_set_tree" in L.smx_last_error() and b"permeability" not in L.smx_last_error()
        mean = np.empty((h, w), np.uint8)
        out = _lib.PairOut(mean_l=mean.ctypes.data)
        assert L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)) == -1
        assert b"mean" in L.smx_last_error() and b"the tree filter" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["sgm"], None))
        assert tp._ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"semi-global" in L.smx_last_error()
        assert b"the tree filter" in L.smx_last_error() and b"permeability" not in L.smx_last_error()
        _lib.check(L.smx_ctx_set_aggregation(ctx, _lib.AGG_MODES["guided"], None))
        _lib.check(L.smx_ctx_set_cross_scale(ctx, C.byref(smx.default_cscale_params())))
        assert tp._ctx_run(ctx, (Il, Ir), None, w, h)[0] == -1 and b"cross-scale" in L.smx_last_error()
        _lib.check(L.smx_ctx_set_cross_scale(ctx, None))
        assert _held(ctx) == 0
        rc, on = tp._ctx_run(ctx, (Il, Ir), None, w, h)                     # and with the conflicts gone it runs
        _lib.check(rc)
        assert _held(ctx) > 0
    finally:
        L.smx_destroy(ctx)
