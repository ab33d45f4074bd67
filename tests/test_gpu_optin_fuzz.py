"""Seeded fuzz of the opt-in stages' device entries against their numpy references: shape, range, parameters, image structure
and the form of the call vary together (tests/fuzz_scenes.py draws them; tests/test_fuzz_scenes_cpu.py proves on the
references what the committed seeds hold).  Twelve seeds per stage, one test id each, and twelve compositions of the stages
through both front ends.  Every output is held bit for bit to the stage's reference (a NaN's payload and sign are not part
of the contract), every buffer lies in a Guarded, workspaces are poisoned before every call and inputs must come back
unchanged.  tools/fuzz_optin.py runs the same cases at other seed bases.

The last section is the table family (fuzz_scenes.table_composition): one option set per seed over every row of the context's
stage table -- twelve aggregation families x five costs, the stages behind the winners drawn on top -- through ONE smx_ctx that
lives across all seeds and through PairPipeline, against the numpy chain of fuzz_scenes.table_reference.  The context gets its
whole option set every time, every setter called, in an order the case draws; every plane, volume and getter of a stage that
ran is compared, every getter of a stage that did not run has to refuse.  test_table_compositions_in_another_order then runs
every case again on the same context in a permuted order: what an earlier option set left behind shows there.

Run on the GPU box:  python -m pytest tests/test_gpu_optin_fuzz.py -m gpu -q --durations=0
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cross_ref
import fuzz_scenes as fs
import subpix_ref
import uniq_ref
from guarded import Guarded
from test_gpu_adcensus import _ap
from test_gpu_census import _cp
from test_gpu_cgf import Call as CgfCall, _p as _cgf_params
from test_gpu_cross import Call as CrossCall, _eq, _p as _cross_params
from test_gpu_sgm import _p as _sgm_params
from test_gpu_speckle import _p as _speckle_params
from test_gpu_subpix import _Path
from test_gpu_wmf import _params as _wmf_params

pytestmark = pytest.mark.gpu

SEEDS = range(fs.SEEDS)
F32 = np.float32
IDENT = np.iinfo(np.int64).max


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(a, n, misalign=0):
    a = np.ascontiguousarray(a)
    return Guarded(a.nbytes, a.dtype, a.shape, plane=n, misalign=misalign).load(a)


def _out(dtype, shape, n, misalign=0):
    dtype = np.dtype(dtype)
    return Guarded(int(np.prod(shape)) * dtype.itemsize, dtype, shape, plane=n, misalign=misalign)


def _ptr(g):
    return None if g is None else g.ptr


class _Bound:
    """smx_set_max_slices_per_launch for the calling thread, restored afterwards."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        _lib.check(smx.lib().smx_set_max_slices_per_launch(self.n))

    def __exit__(self, *a):
        smx.lib().smx_set_max_slices_per_launch(0)


# ---------------------------------------------------------------------------------------------
# the matching costs
# ---------------------------------------------------------------------------------------------
def _census_codes(p, images, per_launch, n):
    """smx_dev_census over the pair, one launch for both images or one each -> (Guarded of the codes, the inputs)"""
    h, w = images[0].shape
    gin = _in(np.stack(images), n, misalign=1)
    codes = _out(np.uint64, (2, h, w), n, misalign=8)
    for first in range(0, 2, per_launch):
        _lib.check(smx.lib().smx_dev_census(C.byref(p), C.c_void_p(gin.ptr.value + first * n), C.c_void_p(codes.ptr.value + 8 * first * n),
                                            w, h, per_launch, _stream()))
    codes.check("d_code")
    gin.check_unchanged("the images")
    return codes


def _cost_outputs(c, n):
    """the guarded volumes of the views the case takes: [left or None, right or None]"""
    shape = (c["s1"] - c["s0"], c["h"], c["w"])
    return [_out(F32, shape, n, misalign=4 * v) if v in fs._views(c["views"]) else None for v in (0, 1)]


def _check_costs(c, out, want, label):
    for v, g in enumerate(out):
        if g is None:
            continue
        if c["s1"] == c["s0"]:
            g.check_untouched(f"{label} view {v}: an empty range launches nothing")
        else:
            g.check(f"{label} view {v}")
            _eq(g.numpy(), want[v], f"{label} cost of view {v}")


def run_census(c):
    w, h, n = c["w"], c["h"], c["w"] * c["h"]
    want = fs.reference("census", c)
    p = _cp(c["rx"], c["ry"], c["th"])
    codes = _census_codes(p, (c["Il"], c["Ir"]), c["per_launch"], n)
    got = codes.numpy().view(np.uint64)
    for v in (0, 1):
        _eq(got[v], want["codes"][v], f"codes of image {v}")
    codes.load(got)
    out = _cost_outputs(c, n)
    _lib.check(smx.lib().smx_dev_census_cost_pair(C.byref(p), codes.ptr, _ptr(out[0]), _ptr(out[1]), w, h, c["dminl"], c["dminr"],
                                                  c["s0"], c["s1"], _stream()))
    _check_costs(c, out, want["cost"], "census")
    codes.check_unchanged("d_code")


def run_adcensus(c):
    import torch
    w, h, n = c["w"], c["h"], c["w"] * c["h"]
    want = fs.reference("adcensus", c)
    p = _ap(c["colour"], c["rx"], c["ry"], c["th"], c["lambda_census"], c["lambda_ad"], c["scale"])
    codes = _census_codes(p.census, c["grays"], 2, n)
    codes.load(codes.numpy())
    tab = _out(F32, (_lib.ADCENSUS_TABLE_FLOATS,), n)
    _lib.check(smx.lib().smx_dev_adcensus_tables(C.byref(p), tab.ptr, _stream()))
    torch.cuda.synchronize()
    tab.check("d_tables")
    tab.load(tab.numpy())
    imgs = [_in(i, n, misalign=1 + v) for v, i in enumerate(c["imgs"])]
    out = _cost_outputs(c, n)
    _lib.check(smx.lib().smx_dev_adcensus_cost_pair(C.byref(p), tab.ptr, codes.ptr, imgs[0].ptr, imgs[1].ptr, c["ch"], _ptr(out[0]),
                                                    _ptr(out[1]), w, h, c["dminl"], c["dminr"], c["s0"], c["s1"], _stream()))
    _check_costs(c, out, want["cost"], "adcensus")
    for g, name in ((codes, "d_code"), (tab, "d_tables"), (imgs[0], "d_img_l"), (imgs[1], "d_img_r")):
        g.check_unchanged(name)


# ---------------------------------------------------------------------------------------------
# the aggregations with a slice range: colour-guided filter, cross
# ---------------------------------------------------------------------------------------------
def _chunked(call, p, c, want_q, label):
    """The drawn calls of a cgf / cross Call over [0, D) on one set of keys -- the first on fresh keys, the later ones
    accumulating -- with the drawn workspace and bound; keys, states and the aggregated slices against the reference."""
    form, n = c["form"], c["w"] * c["h"]
    views = fs._views(form["views"])
    outs = form["outs"]
    pieces = []
    for s0, s1 in form["ranges"]:
        call.agg = _out(F32, (len(views), s1 - s0, c["h"], c["w"]), n)       # (a call's views lie s1 - s0 slices apart)
        call.poison()
        with _Bound(form["bound"]):
            _lib.check(call.run(p, s0, s1, agg=outs["agg"], nbr=outs["nbr"], uq=outs["uq"]))
        call.check_memory()
        if outs["agg"]:
            pieces.append(call.agg.numpy())
        else:
            call.agg.check_untouched("d_agg of a call without it")
    keys, nbr, uq = call.keys.numpy(), call.nbr.numpy(), call.uq.numpy()
    for slot, v in enumerate(views):
        st = want_q["states"][v]
        _eq(keys[slot], st["keys"], f"{label} keys of view {v}")
        if outs["agg"]:
            _eq(np.concatenate([a[slot] for a in pieces]), want_q["q"][v], f"{label} agg of view {v}")
        for name, on, got, g in (("nbr", outs["nbr"], nbr, call.nbr), ("uq", outs["uq"], uq, call.uq)):
            if on:
                _eq(got[slot], st[name], f"{label} {name} of view {v}")
            else:
                g.check_untouched(f"d_{name} of calls without it")


def _view_args(c):
    """(guide_l, cost_l, guide_r, cost_r) with None for the view a one-view case leaves out"""
    views = fs._views(c["form"]["views"])
    pick = lambda a, v: a[v] if v in views else None
    return pick(c["guides"], 0), pick(c["costs"], 0), pick(c["guides"], 1), pick(c["costs"], 1)


def run_cgf(c):
    want = fs.reference("cgf", c)
    call = CgfCall(*_view_args(c), ws_slices=c["form"]["c"])
    _chunked(call, _cgf_params(c["radius"], c["eps"]), c, want, "cgf")


def run_cross(c):
    want = fs.reference("cross", c)
    p = _cross_params(l1=c["l1"], l2=c["l2"], tau1=c["tau1"], tau2=c["tau2"], iterations=c["iterations"])
    n = c["w"] * c["h"]
    gl, _, gr, _ = _view_args(c)
    views = fs._views(c["form"]["views"])
    gg = [None if g is None else _in(g, n, misalign=3) for g in (gl, gr)]
    arms = _out(np.uint8, (len(views) * n * 4,), n, misalign=4)
    _lib.check(smx.lib().smx_dev_cross_arms(C.byref(p), _ptr(gg[0]), _ptr(gg[1]), c["ch"], c["w"], c["h"], arms.ptr, _stream()))
    arms.check("d_arms")
    got = arms.numpy().view(np.uint32).reshape(len(views), c["h"], c["w"])
    for slot, v in enumerate(views):
        _eq(got[slot], cross_ref.pack_arms(want["arms"][v]), f"arms of view {v}")
        gg[v].check_unchanged("a guide")
    call = CrossCall(*_view_args(c), ws_slices=c["form"]["c"])
    _chunked(call, p, c, want, "cross")


# ---------------------------------------------------------------------------------------------
# semi-global matching
# ---------------------------------------------------------------------------------------------
def run_sgm(c):
    D, h, w = c["D"], c["h"], c["w"]
    n = w * h
    want = fs.reference("sgm", c)["views"]
    views, outs = fs._views(c["views"]), c["outs"]
    nv = len(views)
    p = _sgm_params(c["p1"], c["p2"], c["paths"])
    inp = [_in(c["costs"][v], n) if v in views else None for v in (0, 1)]
    keys = _out(np.int64, (nv, h, w), n)
    agg = _out(F32, (nv, D, h, w), n)
    nbr = _out(F32, (nv, 3, h, w), n)
    uq = _out(F32, (nv, 3, h, w), n, misalign=4)
    L = smx.lib()
    ws_bytes = L.smx_sgm_workspace_bytes(w, h, D, nv)
    assert ws_bytes > 0
    ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), misalign=13, fill=0x5A, plane=n)
    ws.view.fill_(0xC3)
    opt = lambda g, on: g.ptr if on else None
    if outs["uq"]:
        rc = L.smx_dev_sgm_wta_pair_uq(C.byref(p), _ptr(inp[0]), _ptr(inp[1]), w, h, D, keys.ptr, opt(agg, outs["agg"]),
                                       opt(nbr, outs["nbr"]), uq.ptr, ws.ptr, ws_bytes, _stream())
    else:
        rc = L.smx_dev_sgm_wta_pair(C.byref(p), _ptr(inp[0]), _ptr(inp[1]), w, h, D, keys.ptr, opt(agg, outs["agg"]),
                                    opt(nbr, outs["nbr"]), ws.ptr, ws_bytes, _stream())
    _lib.check(rc)
    for g, name in ((keys, "d_keys"), (agg, "d_agg"), (nbr, "d_nbr"), (uq, "d_uq"), (ws, "d_ws")):
        g.check(name)
    for v in views:
        inp[v].check_unchanged("d_cost")
    for slot, v in enumerate(views):
        _eq(keys.numpy()[slot], want[v]["keys"], f"sgm keys of view {v}")
        for name, g in (("agg", agg), ("nbr", nbr), ("uq", uq)):
            if outs[name]:
                _eq(g.numpy()[slot], want[v][name], f"sgm {name} of view {v}")
            else:
                g.check_untouched(f"d_{name} of a call without it")


# ---------------------------------------------------------------------------------------------
# the winner-take-all state of the guided-filter aggregation across launches and calls, and what reads it
# ---------------------------------------------------------------------------------------------
def run_wta(c, orc):
    w, h, D = c["w"], c["h"], c["D"]
    n = w * h
    want = fs.reference("wta", c, orc=orc)
    form = c["form"]
    outs = form["outs"]
    p = smx.default_params()
    for k, v in c["params"].items():
        setattr(p, k, v)
    L = smx.lib()
    imgs = [_in(c["Il"], n, misalign=1), _in(c["Ir"], n, misalign=2)]
    keys = _out(np.int64, (2, h, w), n)
    keys.view.fill_(0 if c["fresh"] else IDENT)                # (fresh keys are not read: a loaded 0 would beat every winner)
    nbr = _out(F32, (2, 3, h, w), n, misalign=4)
    uq = _out(F32, (2, 3, h, w), n, misalign=8)
    mean = _out(np.uint8, (2, h, w), n, misalign=1)
    ws_bytes = 2 * L.smx_agg_workspace_bytes(w, h, form["c"])
    ws = Guarded(ws_bytes, np.uint8, (ws_bytes,), misalign=13, fill=0x5A, plane=n)
    pieces = []
    with _Path(c["path"]):
        for i, (s0, s1) in enumerate(form["ranges"]):
            agg = _out(F32, (2, s1 - s0, h, w), n)
            ws.view.fill_(0xC3)
            L.smx_set_keys_fresh(1 if c["fresh"] and i == 0 else 0)
            try:
                with _Bound(form["bound"]):
                    _lib.check(L.smx_dev_aggregate_wta_pair_uq(
                        C.byref(p), imgs[0].ptr, imgs[1].ptr, None, None, w, h, c["dminl"], c["dminr"], s0, s1, keys.ptr,
                        mean.ptr if outs["mean"] else None, agg.ptr if outs["agg"] else None, ws.ptr, ws_bytes,
                        nbr.ptr if outs["nbr"] else None, uq.ptr, _stream()))
            finally:
                L.smx_set_keys_fresh(0)
            for g, name in ((keys, "d_keys"), (nbr, "d_nbr"), (uq, "d_uq"), (mean, "d_mean_u8"), (agg, "d_agg"), (ws, "d_ws")):
                g.check(name)
            _lib.check(L.smx_dev_agg_status(ws.ptr))
            assert L.smx_last_agg_path() == {3: 2}.get(c["path"], c["path"])
            if outs["agg"]:
                pieces.append(agg.numpy())
            else:
                agg.check_untouched("d_agg of a call without it")
    for g in imgs:
        g.check_unchanged("an image")
    for v in (0, 1):
        st = want["states"][v]
        _eq(keys.numpy()[v], st["keys"], f"keys of view {v}")
        _eq(uq.numpy()[v], st["uq"], f"uq of view {v}")
        if outs["nbr"]:
            _eq(nbr.numpy()[v], st["nbr"], f"nbr of view {v}")
        if outs["agg"]:
            _eq(np.concatenate([a[v] for a in pieces]), want["aggl" if v == 0 else "aggr"], f"agg of view {v}")
        if outs["mean"]:
            _eq(mean.numpy()[v], want["meanl" if v == 0 else "meanr"], f"mean of view {v}")
    for g, on, name in ((nbr, outs["nbr"], "d_nbr"), (mean, outs["mean"], "d_mean_u8")):
        if not on:
            g.check_untouched(name + " of calls without it")
    # what reads the state: the sub-pixel fit in both modes and the uniqueness test, on the reference's state and maps
    states = want["states"]
    gk = _in(np.stack([s["keys"] for s in states]), n)
    gn = _in(np.stack([s["nbr"] for s in states]), n)
    dmap = np.stack([want["dmapl"], want["dmapr"]])
    ins = dict(keys=gk, nbr=gn, dmap=_in(dmap, n), occlusion=_in(want["occlusion"], n), filled=_in(want["filled"], n))
    for mode in sorted(subpix_ref.MODES):
        sub, subf = _out(F32, (2, h, w), n, misalign=4), _out(F32, (h, w), n, misalign=8)
        _lib.check(L.smx_dev_subpixel_pair(subpix_ref.MODES[mode], gk.ptr, gn.ptr, ins["dmap"].ptr, ins["occlusion"].ptr,
                                           ins["filled"].ptr, w, h, c["dminl"], sub.ptr, subf.ptr, _stream()))
        sub.check("d_sub")
        subf.check("d_sub_filled")
        for v in (0, 1):
            st = states[v]
            want_sub, wf = subpix_ref.maps(subpix_ref.MODES[mode], st["z"], st["best"], st["nbr"][0], st["nbr"][1], dmap[v],
                                      want["occlusion"] if v == 0 else None, want["filled"], c["dminl"])
            _eq(sub.numpy()[v], want_sub, f"{mode} sub of view {v}")
            if v == 0:
                _eq(subf.numpy(), wf, f"{mode} sub_filled")
    for k, g in ins.items():
        g.check_unchanged("subpixel input " + k)
    has, c0 = uniq_ref.key_fields(states[0]["keys"])
    vmin, new_val = float(c["dminl"]), float(c["dminl"] - 100)
    wu, wm = uniq_ref.apply(want["occlusion"], has, c0, states[0]["uq"][0], c["ratio"], vmin, new_val)
    gs = _in(states[0]["uq"][0], n, misalign=4)
    gk0 = _in(states[0]["keys"], n)
    gu, gm = _out(F32, (h, w), n, misalign=8), _out(F32, (h, w), n, misalign=12)
    _lib.check(L.smx_dev_uniqueness(c["ratio"], gk0.ptr, gs.ptr, ins["occlusion"].ptr, gu.ptr, gm.ptr, w, h, vmin, new_val, _stream()))
    gu.check("d_out")
    gm.check("d_margin")
    _eq(gu.numpy(), wu, "uniqueness map")
    _eq(gm.numpy(), wm, "uniqueness margin")
    for g, name in ((gk0, "d_keys"), (gs, "d_uq"), (ins["occlusion"], "d_disp")):
        g.check_unchanged(name)


# ---------------------------------------------------------------------------------------------
# the refinements of the map
# ---------------------------------------------------------------------------------------------
def run_speckle(c):
    w, h = c["w"], c["h"]
    n = w * h
    want = fs.reference("speckle", c)["out"]
    L = smx.lib()
    need = L.smx_speckle_workspace_bytes(w, h)
    ws = Guarded(need, np.uint8, (need,), misalign=7, fill=0x5A, plane=n)
    ws.view.fill_(0xC3)
    src = _in(c["disp"], n)
    dst = src if c["in_place"] else _out(F32, (h, w), n, misalign=4)
    _lib.check(L.smx_dev_speckle_filter(C.byref(_speckle_params(c["max_size"], c["max_diff"])), src.ptr, dst.ptr, w, h, float(c["dmin"]),
                                        float(c["dmin"] - 100), ws.ptr, need, _stream()))
    dst.check("d_out")
    ws.check("d_ws")
    if not c["in_place"]:
        src.check_unchanged("d_disp")
    _eq(dst.numpy(), want, "speckle")


def run_wmf(c):
    w, h = c["w"], c["h"]
    n = w * h
    p = _wmf_params(c["radius"], c["sigma_s"], c["sigma_c"])
    want = fs.reference("wmf", c, tables=smx.wmf_weights(p))["out"]
    ins = dict(guide=_in(c["guide"], n, misalign=1), disp=_in(c["disp"], n))
    if c["select"] is not None:
        ins["select"] = _in(c["select"], n, misalign=4)
    out = _out(F32, (h, w), n, misalign=8)
    _lib.check(smx.lib().smx_dev_weighted_median(C.byref(p), ins["guide"].ptr, ins["disp"].ptr, _ptr(ins.get("select")), out.ptr, w, h,
                                                 c["dmin"], c["D"], _stream()))
    out.check("d_out")
    for k, g in ins.items():
        g.check_unchanged(k)
    _eq(out.numpy(), want, "weighted median")


def run_permeability(c):
    """tests/test_gpu_perm.py's guarded call: every buffer in a Guarded, the workspace poisoned, inputs unchanged (the volumes
    too unless the call filters in place), what the call must not write untouched, everything else against the reference"""
    from test_gpu_perm import _call
    want = fs.reference("permeability", c)["views"]
    with _Bound(c["bound"]):
        _call(c["costs"], c["guides"], want, c["w"], c["h"], c["D"], c["sigma"], c["views"], c["store"], c["nbr"], c["uq"],
              ws_slices=c["c"])


def run_bp(c):
    """tests/test_gpu_bp.py's guarded call: the drawn views and outputs, the workspace poisoned and misaligned; an output the
    call does not take stays untouched"""
    from test_gpu_bp import Call as BpCall, _p as _bp_params
    views = fs._views(c["views"])
    want = fs.reference("bp", c)["views"]
    call = BpCall(*(c["costs"][v] if v in views else None for v in (0, 1)), levels=c["levels"], misalign=c["misalign"])
    absent = [k for k, on in c["outs"].items() if not on]
    _lib.check(call.run(_bp_params(c["step"], c["trunc"], c["iterations"], c["levels"], c["data_scale"]),
                        **{k: False for k in absent}))
    call.check_memory()
    for slot, v in enumerate(views):
        for g, name in call.outs:
            if name in absent:
                g.check_untouched(f"d_{name} of a call without it")
            else:
                _eq(g.numpy()[slot], want[v][name], f"bp {name} of view {v}")


def run_mi(c):
    """the four device entries of the MI cost, each on guarded buffers: the histogram of the drawn map, its table, the random
    start map, and the drawn slices and views of the cost from the drawn table"""
    import torch
    L = smx.lib()
    w, h, n = c["w"], c["h"], c["w"] * c["h"]
    want = fs.reference("mi", c)
    imgs = [_in(c["Il"], n, misalign=1), _in(c["Ir"], n, misalign=2)]
    disp = _in(c["disp"], n, misalign=4)
    hist = _out(np.uint8, (256 * 256 * 4,), n)          # (the 256 x 256 uint32 counters, as bytes)
    _lib.check(L.smx_dev_mi_histogram(imgs[0].ptr, imgs[1].ptr, disp.ptr, float(c["mark"]), hist.ptr, w, h, _stream()))
    hist.check("d_hist")
    H = np.ascontiguousarray(hist.numpy()).view(np.uint32).reshape(256, 256)
    _eq(H, want["hist"], "histogram")
    tab = _out(np.uint8, (256, 256), n)          # (the table is read 16 bytes at a time)
    _lib.check(L.smx_dev_mi_table(H.ctypes.data, tab.ptr, _stream()))
    torch.cuda.synchronize()
    tab.check("d_table")
    _eq(tab.numpy(), want["learned"], "table")
    rmap = _out(F32, (h, w), n, misalign=8)
    _lib.check(L.smx_dev_mi_random_map(rmap.ptr, w, h, c["dminl"], c["D"], c["map_seed"], _stream()))
    rmap.check("d_map")
    _eq(rmap.numpy(), want["random_map"], "random map")
    tab.load(want["table"])
    out = _cost_outputs(c, n)
    _lib.check(L.smx_dev_mi_cost_pair(tab.ptr, imgs[0].ptr, imgs[1].ptr, _ptr(out[0]), _ptr(out[1]), w, h, c["dminl"],
                                      c["dminr"], c["s0"], c["s1"], _stream()))
    _check_costs(c, out, want["cost"], "mi")
    for g, name in ((tab, "d_table"), (imgs[0], "d_img_l"), (imgs[1], "d_img_r"), (disp, "d_map")):
        g.check_unchanged(name)


def run_patchmatch(c):
    """tests/test_gpu_patchmatch.py's guarded call: the search with its four outputs, or the cost of the drawn planes alone
    (planes unchanged, disp and label untouched); the workspace poisoned and misaligned"""
    from test_gpu_patchmatch import Call as PmCall
    want = fs.reference("patchmatch", c)
    pm = _struct(_lib.default_pm_params(), **c["pm"])
    search = c["entry"] == "search"
    call = PmCall(c["left"], c["right"], c["D"], c["dminl"], c["dminr"], c["misalign"], planes=None if search else c["planes"])
    _lib.check(call.search(pm) if search else call.cost(pm))
    call.check_memory(planes_in=not search)
    got = call.results()
    for k in ("planes", "cost", "disp", "label") if search else ("cost",):
        a, b = np.ascontiguousarray(got[k], F32).view(np.uint32), np.ascontiguousarray(want[k], F32).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), f"patchmatch {k}: {int((a != b).sum())} values differ"
    if not search:
        for k in ("disp", "label"):
            call.out[k].check_untouched(f"d_{k} of the plane cost")


RUN = dict(census=run_census, adcensus=run_adcensus, cgf=run_cgf, cross=run_cross, sgm=run_sgm, wta=run_wta, speckle=run_speckle,
           wmf=run_wmf, permeability=run_permeability, bp=run_bp, mi=run_mi, patchmatch=run_patchmatch)


def run(stage, seed, base=None, orc=None):
    """one drawn case through its device entries; AssertionError with the first difference"""
    c = fs.draw(stage, seed, base)
    with np.errstate(all="ignore"):
        RUN[stage](c, orc) if stage == "wta" else RUN[stage](c)
    return c


@pytest.mark.parametrize("seed", SEEDS)
def test_census_fuzz(seed):
    run("census", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_adcensus_fuzz(seed):
    run("adcensus", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_colour_guided_filter_fuzz(seed):
    run("cgf", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_cross_fuzz(seed):
    run("cross", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_sgm_fuzz(seed):
    run("sgm", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_wta_state_fuzz(orc, seed):
    run("wta", seed, orc=orc)


@pytest.mark.parametrize("seed", SEEDS)
def test_speckle_fuzz(seed):
    run("speckle", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_weighted_median_fuzz(seed):
    run("wmf", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_permeability_fuzz(seed):
    run("permeability", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_bp_fuzz(seed):
    run("bp", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_mi_fuzz(seed):
    run("mi", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_patchmatch_fuzz(seed):
    run("patchmatch", seed)


# ---------------------------------------------------------------------------------------------
# compositions: one drawn option set through PairPipeline, through one smx_ctx, and through the numpy chain
# ---------------------------------------------------------------------------------------------
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _option_params(c):
    o = c["opt"]
    p = smx.default_params()
    p.radius, p.eps = c["radius"], c["eps"]
    spk = _speckle_params(*o["speckle"]) if o["speckle"] else None
    ap = _ap(int(o["cost"] == "adcensus colour"), o["census"]["rx"], o["census"]["ry"], o["census"]["th"],
             o["adcensus"]["lambda_census"], o["adcensus"]["lambda_ad"], o["adcensus"]["scale"])
    return dict(p=p, spk=spk, ap=ap, cp=_cp(**o["census"]), sp=_sgm_params(**o["sgm"]), xp=_cross_params(**o["cross"]),
                ratio=fs.ratio_of(o["uniqueness"]) if o["uniqueness"] else None)


def _through_the_pipeline(c, want, P):
    from stereo_matching_cuda_amd.device import PairPipeline
    o = c["opt"]
    pipe = PairPipeline(c["w"], c["h"], c["D"], dminl=c["dminl"], dminr=c["dminr"], params=P["p"], want_agg=True,
                        slices_in_flight=o["sif"], cost={"reference": None, "census": "census"}.get(o["cost"], "adcensus"),
                        census_params=P["cp"], adcensus_params=P["ap"],
                        aggregation={"sgm": "sgm", "cross": "cross", "cross rgb": "cross"}.get(o["agg"]),
                        guidance="rgb" if o["agg"] == "guided rgb" else None, sgm_params=P["sp"], cross_params=P["xp"],
                        subpixel=o["subpixel"], uniqueness=P["ratio"], speckle=P["spk"], wmf=o["wmf"])
    colour = o["agg"] in ("guided rgb", "cross rgb") or o["cost"] == "adcensus colour"
    kw = dict(rgb_l=_t(c["rgb"][0]), rgb_r=_t(c["rgb"][1])) if colour else {}
    pipe.run(_t(want["grayl"]), _t(want["grayr"]), **kw)
    got = pipe.results()
    keys = ["aggl", "aggr", "bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled"]
    keys += ["unique"] * bool(o["uniqueness"]) + ["despeckled"] * bool(o["speckle"]) + ["refined"] * bool(o["wmf"])
    keys += ["subpixl", "subpixr", "subpix_filled"] * bool(o["subpixel"])
    for k in keys:
        _eq(got[k], want[k], "pipeline " + k)
    _eq(pipe.keys.cpu().numpy(), want["keys"], "pipeline keys")
    return got


def _through_the_context(ctx, c, want, P):
    L, o = smx.lib(), c["opt"]
    h, w, D = c["h"], c["w"], c["D"]
    # the whole option set, every time: what is not drawn is switched off
    _lib.check(L.smx_ctx_set_adcensus(ctx, None))
    _lib.check(L.smx_ctx_set_cost(ctx, 1 if o["cost"] == "census" else 0, C.byref(P["cp"]) if o["cost"] == "census" else None))
    if o["cost"].startswith("adcensus"):
        _lib.check(L.smx_ctx_set_adcensus(ctx, C.byref(P["ap"])))
    _lib.check(L.smx_ctx_set_aggregation(ctx, 1 if o["agg"] == "sgm" else 0, C.byref(P["sp"]) if o["agg"] == "sgm" else None))
    _lib.check(L.smx_ctx_set_cross(ctx, C.byref(P["xp"]) if o["agg"].startswith("cross") else None))
    _lib.check(L.smx_ctx_set_guidance(ctx, 1 if o["agg"] == "guided rgb" else 0))
    _lib.check(L.smx_ctx_set_subpixel(ctx, subpix_ref.MODES[o["subpixel"]] if o["subpixel"] else 0))
    _lib.check(L.smx_ctx_set_uniqueness(ctx, P["ratio"] or 0.0))
    _lib.check(L.smx_ctx_set_speckle(ctx, C.byref(P["spk"]) if P["spk"] else None))
    bufs = {k: np.empty((h, w), F32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    if o["volumes"]:
        bufs.update({k: np.empty((D, h, w), F32) for k in ("agg_l", "agg_r", "cost_l", "cost_r")})
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    colour = o["agg"] in ("guided rgb", "cross rgb") or o["cost"] == "adcensus colour"
    with _Bound(o["bound"]):
        if colour:
            rc = L.smx_ctx_stereo_pair_rgb(ctx, c["rgb"][0].ctypes.data, c["rgb"][1].ctypes.data, c["ch"], c["dminl"], c["dminr"],
                                           C.byref(out))
        else:
            rc = L.smx_ctx_stereo_pair(ctx, want["grayl"].ctypes.data, want["grayr"].ctypes.data, c["dminl"], c["dminr"], C.byref(out))
    _lib.check(rc)
    for k, v in bufs.items():
        _eq(v, want[k.replace("_", "")], "context " + k)
    maps = {}
    if o["subpixel"]:
        sub = [np.empty((h, w), F32) for _ in range(3)]
        _lib.check(L.smx_ctx_subpixel_maps(ctx, *(s.ctypes.data for s in sub)))
        maps.update(zip(("subpixl", "subpixr", "subpix_filled"), sub))
    if o["uniqueness"]:
        maps["unique"] = np.empty((h, w), F32)
        _lib.check(L.smx_ctx_uniqueness_map(ctx, maps["unique"].ctypes.data, None))
    if o["speckle"]:
        maps["despeckled"] = np.empty((h, w), F32)
        _lib.check(L.smx_ctx_speckle_map(ctx, maps["despeckled"].ctypes.data))
    for k, v in maps.items():
        _eq(v, want[k], "context " + k)
    return dict(bufs, **maps)


@pytest.fixture(scope="module")
def context():
    """one context for the twelve compositions: a setting left over from the draw before cannot hide"""
    s = fs.composition_setup()
    p = smx.default_params()
    p.radius, p.eps = s["radius"], s["eps"]
    ctx = C.c_void_p()
    _lib.check(smx.lib().smx_create(C.byref(p), s["w"], s["h"], s["D"], C.byref(ctx)))
    yield ctx
    smx.lib().smx_destroy(ctx)


def run_composition(seed, ctx, orc, base=None):
    c = fs.composition(seed, base)
    want = fs.composition_reference(c, orc)
    P = _option_params(c)
    pipe = _through_the_pipeline(c, want, P)
    got = _through_the_context(ctx, c, want, P)
    for k, v in got.items():            # and the two front ends against each other
        name = k.replace("_", "") if k in ("best_l", "best_r", "dmap_l", "dmap_r", "agg_l", "agg_r") else k
        if name in pipe:
            _eq(v, pipe[name], f"context against pipeline {k}")
    return c


@pytest.mark.parametrize("seed", SEEDS)
def test_composition_fuzz(orc, context, seed):
    with np.errstate(all="ignore"):
        run_composition(seed, context, orc)


# ---------------------------------------------------------------------------------------------
# the table family: one option set per seed over every row of the context's stage table (fuzz_scenes.table_composition)
# through ONE smx_ctx and through PairPipeline, against the numpy chain; then every case again on the same context in
# another order
# ---------------------------------------------------------------------------------------------
TABLE_SEEDS = range(fs.TABLE_SEEDS)
E_ARG = -1          # SMX_E_ARG


def _struct(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _table_params(c):
    """the parameter structs of every stage of the case, those of the stages that are off included (None: nothing drawn)"""
    o = c["opt"]
    p = smx.default_params()
    p.radius, p.eps = c["radius"], c["eps"]
    vote = o["vote"]
    P = dict(p=p, cp=_cp(**o["census"]),
             ap=_ap(int(o["cost"] == "adcensus colour"), o["census"]["rx"], o["census"]["ry"], o["census"]["th"],
                    o["adcensus"]["lambda_census"], o["adcensus"]["lambda_ad"], o["adcensus"]["scale"]),
             mp=_struct(_lib.default_mi_params(), **o["mi"]) if o["mi"] else None,
             sp=_sgm_params(**o["sgm"]), xp=_cross_params(**o["cross"]),
             so=_struct(_lib.default_scanline_params(), **o["scanline"]),
             bp=_struct(_lib.default_bp_params(), **o["bp"]), pm=_struct(_lib.default_pm_params(), **o["patchmatch"]),
             cs=_struct(_lib.default_cscale_params(), **o["cross_scale"]) if o["cross_scale"] else None,
             perm=_struct(_lib.default_perm_params(), **o["permeability"]) if o["permeability"] else None,
             spk=_speckle_params(*o["speckle"]) if o["speckle"] else None,
             ratio=fs.ratio_of(o["uniqueness"]) if o["uniqueness"] else None,
             vp=_struct(_lib.default_vote_params(), tau_s=vote["params"]["tau_s"], tau_h_pct=vote["params"]["tau_h_pct"],
                        iterations=vote["params"]["iterations"], interpolate=vote["params"]["interpolate_"]) if vote else None,
             va=_cross_params(iterations=1, **vote["arms"]) if vote else None,
             adj=_struct(_lib.default_adjust_params(), **o["adjust"]) if o["adjust"] else None)
    return P


def _set_the_whole_option_set(ctx, c, P):
    """every setter of the context, the stages that are off included, in the order the case draws
    (fuzz_scenes.table_applied_order)"""
    L, o = smx.lib(), c["opt"]
    agg = fs.FAMILIES[o["family"]][0]
    ref_or_null = lambda on, p: C.byref(p) if on else None
    cost = o["cost"]
    calls = {
        "cost": lambda: L.smx_ctx_set_cost(ctx, 1 if cost == "census" else 0, ref_or_null(cost == "census", P["cp"])),
        "adcensus": lambda: L.smx_ctx_set_adcensus(ctx, ref_or_null(cost.startswith("adcensus"), P["ap"])),
        "mi": lambda: L.smx_ctx_set_mi(ctx, ref_or_null(cost == "mi", P["mp"])),
        "aggregation": lambda: L.smx_ctx_set_aggregation(ctx, 1 if agg == "sgm" else 0, ref_or_null(agg == "sgm", P["sp"])),
        "guidance": lambda: L.smx_ctx_set_guidance(ctx, int(fs.FAMILIES[o["family"]][1])),
        "cross": lambda: L.smx_ctx_set_cross(ctx, ref_or_null(agg in ("cross", "cross-scanline"), P["xp"])),
        "scanline": lambda: L.smx_ctx_set_scanline(ctx, ref_or_null(agg in ("scanline", "cross-scanline"), P["so"])),
        "bp": lambda: L.smx_ctx_set_bp(ctx, ref_or_null(agg == "bp", P["bp"])),
        "patchmatch": lambda: L.smx_ctx_set_patchmatch(ctx, ref_or_null(agg == "patchmatch", P["pm"])),
        "cross_scale": lambda: L.smx_ctx_set_cross_scale(ctx, ref_or_null(P["cs"] is not None, P["cs"])),
        "permeability": lambda: L.smx_ctx_set_permeability(ctx, ref_or_null(P["perm"] is not None, P["perm"])),
        "subpixel": lambda: L.smx_ctx_set_subpixel(ctx, subpix_ref.MODES[o["subpixel"]] if o["subpixel"] else 0),
        "uniqueness": lambda: L.smx_ctx_set_uniqueness(ctx, P["ratio"] or 0.0),
        "speckle": lambda: L.smx_ctx_set_speckle(ctx, ref_or_null(P["spk"] is not None, P["spk"])),
        "vote": lambda: L.smx_ctx_set_vote(ctx, ref_or_null(P["vp"] is not None, P["vp"]),
                                           ref_or_null(P["va"] is not None, P["va"])),
        "adjust": lambda: L.smx_ctx_set_adjust(ctx, ref_or_null(P["adj"] is not None, P["adj"])),
    }
    assert sorted(calls) == sorted(fs.TABLE_SETTERS)
    order = fs.table_applied_order(c)
    for k in order:
        _lib.check(calls[k]())
    return order


TABLE_PLANES = ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")
TABLE_VOLUMES = ("agg_l", "agg_r", "cost_l", "cost_r")


def _through_the_table_context(ctx, c, want, P):
    L, o = smx.lib(), c["opt"]
    h, w, D = c["h"], c["w"], c["D"]
    pm = fs.FAMILIES[o["family"]][0] == "patchmatch"
    _set_the_whole_option_set(ctx, c, P)
    bufs = {k: np.empty((h, w), F32) for k in TABLE_PLANES}
    if o["volumes"]:
        bufs.update({k: np.empty((D, h, w), F32) for k in TABLE_VOLUMES})
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    imgs = c["rgb"] if c["entry"] == "rgb" else (want["grayl"], want["grayr"])
    before = [i.copy() for i in imgs]
    with _Bound(o["bound"]):
        if c["entry"] == "rgb":
            rc = L.smx_ctx_stereo_pair_rgb(ctx, imgs[0].ctypes.data, imgs[1].ctypes.data, c["ch"], c["dminl"], c["dminr"],
                                           C.byref(out))
        else:
            rc = L.smx_ctx_stereo_pair(ctx, imgs[0].ctypes.data, imgs[1].ctypes.data, c["dminl"], c["dminr"], C.byref(out))
    _lib.check(rc)
    for a, b in zip(imgs, before):
        assert a.tobytes() == b.tobytes(), "the context changed a host image"
    for k, v in bufs.items():
        _eq(v, want[k.replace("_", "")], "context " + k)
    plane = lambda: np.empty((h, w), F32)
    got = dict(bufs)

    def getter(ran, entry, names, arrays, *extra):
        """the maps of a stage that ran against the chain; SMX_E_ARG from the getter of a stage that did not"""
        rc = getattr(L, entry)(ctx, *(a.ctypes.data for a in arrays), *extra)
        if not ran:
            assert rc == E_ARG, f"{entry} after a pair without its stage: {rc}"
            return
        _lib.check(rc)
        for k, a in zip(names, arrays):
            _eq(a, want[k], f"context {entry} {k}")
            got[k] = a

    getter(bool(o["subpixel"]), "smx_ctx_subpixel_maps", ("subpixl", "subpixr", "subpix_filled"), [plane() for _ in range(3)])
    getter(bool(o["uniqueness"]), "smx_ctx_uniqueness_map", ("unique", "margin"), [plane(), plane()])
    getter(bool(o["speckle"]), "smx_ctx_speckle_map", ("despeckled",), [plane()])
    getter(bool(o["vote"]), "smx_ctx_vote_map", ("voted",), [plane()])
    getter(o["cost"] == "mi", "smx_ctx_mi_table", ("mi_table", "mi_hist"),
           [np.empty((256, 256), np.uint8), np.empty((256, 256), np.uint32)])
    if pm:
        maps = [np.empty((3, h, w), F32), np.empty((3, h, w), F32), plane(), plane(), plane()]
        _lib.check(L.smx_ctx_patchmatch_maps(ctx, *(m.ctypes.data for m in maps)))
        _eq(np.stack(maps[:2]), want["pm_planes"], "context smx_ctx_patchmatch_maps planes")
        for k, a in zip(("subpixl", "subpixr", "subpix_filled"), maps[2:]):
            _eq(a, want[k], f"context smx_ctx_patchmatch_maps {k}")
            got[k] = a
        got["pm_planes"] = np.stack(maps[:2])
    else:
        assert L.smx_ctx_patchmatch_maps(ctx, None, None, None, None, None) == E_ARG
    return got


def _through_the_table_pipeline(c, want, P):
    from stereo_matching_cuda_amd.device import PairPipeline
    o = c["opt"]
    agg, cgf, _ = fs.FAMILIES[o["family"]]
    pm = agg == "patchmatch"
    kw = dict(dminl=c["dminl"], dminr=c["dminr"], params=P["p"], want_agg=not pm, slices_in_flight=o["sif"],
              cost={"reference": None, "census": "census", "mi": "mi"}.get(o["cost"], "adcensus"), census_params=P["cp"],
              adcensus_params=P["ap"], aggregation=None if agg == "guided" else agg, guidance="rgb" if cgf else None,
              sgm_params=P["sp"], cross_params=P["xp"], subpixel=o["subpixel"], uniqueness=P["ratio"], speckle=P["spk"],
              wmf=o["wmf"],
              vote=P["vp"], vote_arms=P["va"], adjust=P["adj"], cross_scale=P["cs"], permeability=P["perm"])
    for name, on, p in (("mi_params", o["cost"] == "mi", P["mp"]), ("bp_params", agg == "bp", P["bp"]),
                        ("scanline_params", agg in ("scanline", "cross-scanline"), P["so"]), ("pm_params", pm, P["pm"])):
        if on:
            kw[name] = p
    pipe = PairPipeline(c["w"], c["h"], c["D"], **kw)
    colour = fs.table_guides(c, "pipeline")["came"]
    rgb = dict(rgb_l=_t(c["rgb"][0]), rgb_r=_t(c["rgb"][1])) if colour else {}
    ins = [_t(want["grayl"]), _t(want["grayr"])] + list(rgb.values())
    keep = [t.clone() for t in ins]
    pipe.run(ins[0], ins[1], **rgb)
    got = pipe.results()
    import torch
    for a, b in zip(ins, keep):
        assert torch.equal(a, b), "the pipeline changed an input"
    keys = ["bestl", "bestr", "dmapl", "dmapr", "occlusion", "filled"] + ["aggl", "aggr"] * (not pm)
    keys += ["unique", "margin"] * bool(o["uniqueness"]) + ["despeckled"] * bool(o["speckle"]) + ["voted"] * bool(o["vote"])
    keys += ["adjusted"] * bool(o["adjust"]) + ["refined"] * bool(o["wmf"]) + ["pm_planes"] * pm
    keys += ["subpixl", "subpixr", "subpix_filled"] * bool(o["subpixel"] or pm)
    for k in keys:
        _eq(got[k], want[k], "pipeline " + k)
    if not pm:
        _eq(pipe.keys.cpu().numpy(), want["keys"], "pipeline keys")
    if o["cost"] == "mi":
        _eq(pipe.mi_hist.cpu().numpy().view(np.uint32).reshape(256, 256), want["mi_hist"], "pipeline mi_hist")
        _eq(pipe.mi_table.cpu().numpy().reshape(256, 256), want["mi_table"], "pipeline mi_table")
    return got


def create_table_context(base=None):
    s = fs.table_setup(base)
    p = smx.default_params()
    p.radius, p.eps = s["radius"], s["eps"]
    ctx = C.c_void_p()
    _lib.check(smx.lib().smx_create(C.byref(p), s["w"], s["h"], s["D"], C.byref(ctx)))
    return ctx


@pytest.fixture(scope="module")
def table_context():
    """one context for every table composition and for the second pass over them: its buffers only grow, its cross-scale
    children live from pair to pair, and a setting left over from whichever case ran before cannot hide"""
    ctx = create_table_context()
    yield ctx
    smx.lib().smx_destroy(ctx)


_TABLE = {}          # (base, seed) -> (the case, the chain, what the context gave the first time)


def _table_case(seed, orc, base=None):
    if (base, seed) not in _TABLE:
        c = fs.table_composition(seed, base)
        _TABLE[base, seed] = [c, fs.table_reference(c, orc), None]
    return _TABLE[base, seed]


def run_table_composition(seed, ctx, orc, base=None):
    entry = _table_case(seed, orc, base)
    c, want = entry[:2]
    P = _table_params(c)
    # (PairPipeline's vote takes the colour image only where its aggregation took the colour pair: fuzz_scenes.table_guides)
    differs = bool(c["opt"]["vote"]) and fs.table_guides(c, "pipeline")["vote"] != fs.table_guides(c)["vote"]
    pipe = _through_the_table_pipeline(c, fs.table_behind(c, orc, dict(want), "pipeline") if differs else want, P)
    got = _through_the_table_context(ctx, c, want, P)
    entry[2] = got
    names = dict(best_l="bestl", best_r="bestr", dmap_l="dmapl", dmap_r="dmapr", agg_l="aggl", agg_r="aggr")
    behind_the_vote = ("voted", "filled", "subpix_filled") if differs else ()
    for k, v in got.items():            # and the two front ends against each other
        if names.get(k, k) in pipe and k not in behind_the_vote:
            _eq(v, pipe[names.get(k, k)], f"context against pipeline {k}")
    return c


def run_table_again(seed, ctx, orc, base=None):
    """the case once more on the context as it stands: the chain's bits, which are the bits of the first time"""
    c, want, first = _table_case(seed, orc, base)
    got = _through_the_table_context(ctx, c, want, _table_params(c))
    for k, v in (first or {}).items():
        _eq(got[k], v, f"{k} of the second pass against the first")


@pytest.mark.parametrize("seed", TABLE_SEEDS)
def test_table_composition_fuzz(orc, table_context, seed):
    with np.errstate(all="ignore"):
        run_table_composition(seed, table_context, orc)


def test_table_compositions_in_another_order(orc, table_context):
    with np.errstate(all="ignore"):
        for seed in fs.table_order():
            try:
                run_table_again(seed, table_context, orc)
            except AssertionError as e:
                raise AssertionError(f"seed {seed} ({fs.table_composition(seed)['text']}): {e}") from e
