"""Seeded fuzz of the opt-in stages' device entries against their numpy references: shape, range, parameters, image structure
and the form of the call vary together (tests/fuzz_scenes.py draws them; tests/test_fuzz_scenes_cpu.py proves on the
references what the committed seeds hold).  Twelve seeds per stage, one test id each, and twelve compositions of the stages
through both front ends (the last section).  Every output is held bit for bit to the stage's reference (a NaN's payload and sign are not part of the contract), every buffer lies in a Guarded, workspaces are
poisoned before every call and inputs must come back unchanged.  tools/fuzz_optin.py runs the same cases at other seed bases.

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


RUN = dict(census=run_census, adcensus=run_adcensus, cgf=run_cgf, cross=run_cross, sgm=run_sgm, wta=run_wta, speckle=run_speckle,
           wmf=run_wmf)


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
