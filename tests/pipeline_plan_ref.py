"""What PairPipeline and ShardedPair refuse, own and size, as their constructors stated it before they had a stage table.

This is PairPipeline.__init__ (stereo_matching_cuda_amd/device.py) and ShardedPair.__init__ (sharded.py) transcribed statement
for statement as of commit 6a428ae ("Fuzz every row of the context's stage table on one context"), in the order of those
files, without torch: where the constructor allocated a tensor, the transcription records (shape, dtype, zeroed), and where it
queried a workspace size it asks `lib`, anything that answers the smx_*_workspace_bytes / smx_agg_workspace_bytes[_for] /
smx_cscale_level host functions.  It is the reference of tests/test_pipeline_plan_cpu.py and is not derived from
stereo_matching_cuda_amd/pipeline_plan.py: a rule that moves there shows as a difference here.

Where the constructor raised, `refuse` records (the keywords concerned, the kind) and the walk goes on, as Chain.refuse of
ctx_plan_ref.py does, so that a point keeps every refusal that applies to it, in the order of the constructor; the verdict is
"some refusal applies", and the first one is what the old code reported.  The few places where going on needs a usable value
after a refusal (a wrong-typed struct whose fields the next statement reads) say so.

Kinds: "value" (not one of the accepted values or types), "range" (a parameter out of its range), "belongs" (a *_params
keyword without its stage), "conflict" (two options that do not run together), "slices" (a slice sub-range), "shape" (a size
the stage does not take), "budget" (more than max_ws_bytes), "level" (a cross-scale level narrower than 2 pixels), "sharded"
(not part of the sharded driver), "world" (needs world == 1).
"""
import ctypes as C

from stereo_matching_cuda_amd import _lib

U8, I32, I64, F32 = "uint8", "int32", "int64", "float32"
INF = float("inf")


def pipeline(lib, w, h, size_d, dminl=None, dminr=0, s_begin=0, s_end=None,
             slices_in_flight=None, want_agg=False, params=None, max_ws_bytes=64 << 30, multi_kernel=False,
             wmf=None, wmf_params=None, subpixel=None, cost=None, census_params=None, speckle=None,
             aggregation=None, sgm_params=None, bp_params=None, uniqueness=None, guidance=None, adcensus_params=None, mi_params=None,
             cross_params=None, vote=None, vote_arms=None, scanline_params=None, adjust=None, cross_scale=None, pm_params=None,
             permeability=None):
    """-> ("refused", [((keyword, ...), kind), ...]) or ("ok", the outcome as a dict: the attributes the constructor set that
    are plain values under "options", the byte counts under "bytes", the buffers under "buffers" (attribute -> None or (shape,
    dtype, zeroed); cs_gray / cs_rgb are lists of those) and the levels under "levels" (what the constructor handed each level
    pipeline, and that pipeline's outcome))."""
    R = []

    def refuse(kind, *keywords):
        R.append((keywords, kind))

    sub_range = int(s_begin) != 0 or (s_end is not None and int(s_end) != int(size_d))
    if permeability is not None and permeability is not True and not isinstance(permeability, _lib.PermParams):
        refuse("value", "permeability")
        permeability = True                 # (to go on)
    if isinstance(permeability, _lib.PermParams) and not (0.0 < permeability.sigma < INF):
        refuse("range", "permeability")
    if permeability is not None:
        if aggregation is not None:
            refuse("conflict", "permeability", "aggregation")
        if cross_scale is not None:
            refuse("conflict", "permeability", "cross_scale")
        if sub_range:
            refuse("slices", "permeability")
        want_agg = True
    pm = aggregation == "patchmatch"
    if pm_params is not None and not pm:
        refuse("belongs", "pm_params", "aggregation")
    if pm:
        if pm_params is not None and not isinstance(pm_params, _lib.PMParams):
            refuse("value", "pm_params")
            pm_params = None                # (to go on)
        q = pm_params
        if q is not None and not (0 <= q.radius <= 17 and 0.0 < q.gamma < INF and 1 <= q.iterations <= 16 and
                                  0.0 <= q.max_slope <= 8.0):
            refuse("range", "pm_params")
        for name, value in (("cost", cost), ("guidance", guidance), ("cross_scale", cross_scale), ("adjust", adjust),
                            ("uniqueness", uniqueness), ("subpixel", subpixel), ("want_agg", want_agg or None)):
            if value is not None:
                refuse("conflict", "aggregation", name)
        if sub_range:
            refuse("slices", "aggregation")
    if cross_scale is not None and cross_scale is not True and not isinstance(cross_scale, _lib.CScaleParams):
        refuse("value", "cross_scale")
        cross_scale = True                  # (to go on)
    if isinstance(cross_scale, _lib.CScaleParams) and not (1 <= cross_scale.scales <= 5 and 0.0 <= cross_scale.lambda_ < INF):
        refuse("range", "cross_scale")
        cross_scale = True                  # (to go on: the level loop below reads .scales)
    if cross_scale is not None:
        if aggregation is not None:
            refuse("conflict", "cross_scale", "aggregation")
        if sub_range:
            refuse("slices", "cross_scale")
        want_agg = True
    if adjust is not None and adjust is not True and not isinstance(adjust, _lib.AdjustParams):
        refuse("value", "adjust")
        adjust = True                       # (to go on)
    if isinstance(adjust, _lib.AdjustParams) and not (1 <= adjust.tau_e <= 512 and adjust.vertical in (0, 1) and
                                                      1 <= adjust.iterations <= 8):
        refuse("range", "adjust")
    if adjust is not None:
        if sub_range:
            refuse("slices", "adjust")
        if not 1 <= int(size_d) <= 512:
            refuse("shape", "adjust")
    if guidance not in (None, "rgb"):
        refuse("value", "guidance")
    if guidance and aggregation:
        refuse("conflict", "guidance", "aggregation")
    if uniqueness is not None:
        try:
            uniqueness = float(uniqueness)
        except ValueError:                  # (float("abc") is a ValueError of its own)
            refuse("value", "uniqueness")
            uniqueness = 1.0                # (to go on)
        if not (0.0 < uniqueness < INF):
            refuse("value", "uniqueness")
        if sub_range:
            refuse("slices", "uniqueness")
    if aggregation not in (None, "sgm", "bp", "cross", "scanline", "cross-scanline", "patchmatch"):
        refuse("value", "aggregation")
    sgm, cross = aggregation == "sgm", aggregation in ("cross", "cross-scanline")
    bp = aggregation == "bp"
    if bp_params is not None and not bp:
        refuse("belongs", "bp_params", "aggregation")
    so = aggregation in ("scanline", "cross-scanline")
    if scanline_params is not None and not so:
        refuse("belongs", "scanline_params", "aggregation")
    if cost not in (None, "census", "adcensus", "mi"):
        refuse("value", "cost")
    if mi_params is not None and cost != "mi":
        refuse("belongs", "mi_params", "cost")
    if cost == "mi":
        if aggregation == "patchmatch":
            refuse("conflict", "cost", "aggregation")
        if sub_range:
            refuse("slices", "cost")
    if wmf not in (None, "occluded", "all"):
        refuse("value", "wmf")
    if subpixel is not None and subpixel not in _lib.SUBPIX_MODES:
        refuse("value", "subpixel")
    if speckle is not None and speckle is not True and not isinstance(speckle, _lib.SpeckleParams):
        refuse("value", "speckle")
        speckle = True                      # (to go on)
    if vote is not None and vote is not True and not isinstance(vote, _lib.VoteParams):
        refuse("value", "vote")
        vote = True                         # (to go on)
    if vote_arms is not None and not isinstance(vote_arms, _lib.CrossParams):
        refuse("value", "vote_arms")
    if vote_arms is not None and vote is None:
        refuse("belongs", "vote_arms", "vote")
    if not isinstance(vote_arms, _lib.CrossParams):
        vote_arms = None                    # (to go on)
    o, by, buf = {}, {}, {}
    o["w"], o["h"], o["size_d"] = int(w), int(h), int(size_d)
    w, h, size_d = o["w"], o["h"], o["size_d"]
    n = o["n"] = w * h
    dminl = o["dminl"] = -(size_d - 1) if dminl is None else int(dminl)
    dminr = o["dminr"] = int(dminr)
    s_begin = o["s_begin"] = int(s_begin)
    s_end = o["s_end"] = size_d if s_end is None else int(s_end)
    params = o["params"] = params if params is not None else _lib.default_params()
    o["aggregation"] = aggregation
    o["adjust"] = buf["adjusted"] = buf["adjust_ws"] = None
    by["adjust_ws_bytes"] = 0
    if adjust is not None:
        by["adjust_ws_bytes"] = int(lib.smx_adjust_workspace_bytes(w, h))
        if by["adjust_ws_bytes"] == 0:
            refuse("shape", "adjust")
        held = 2 * size_d * n * 4 + by["adjust_ws_bytes"]
        if held > max_ws_bytes:
            refuse("budget", "adjust")
        max_ws_bytes -= held                # what is left for the aggregation
        want_agg = True
        o["adjust"] = _lib.default_adjust_params() if adjust is True else adjust
    o["sgm_params"] = buf["sgm_cost"] = buf["sgm_ws"] = None
    by["sgm_ws_bytes"] = 0
    if sgm:
        if s_begin != 0 or s_end != size_d:
            refuse("slices", "aggregation")
        o["sgm_params"] = sgm_params if sgm_params is not None else _lib.default_sgm_params()
        by["sgm_ws_bytes"] = int(lib.smx_sgm_workspace_bytes(w, h, size_d, 2))
        if by["sgm_ws_bytes"] == 0:
            refuse("shape", "aggregation")
        if by["sgm_ws_bytes"] + 2 * size_d * n * 4 > max_ws_bytes:
            refuse("budget", "aggregation")
    o["bp_params"] = buf["bp_cost"] = buf["bp_ws"] = None
    by["bp_ws_bytes"] = 0
    if bp:
        if s_begin != 0 or s_end != size_d:
            refuse("slices", "aggregation")
        o["bp_params"] = bp_params if bp_params is not None else _lib.default_bp_params()
        q = o["bp_params"]
        if not (0 <= q.step <= 4095 and 0 <= q.trunc <= 4095 and 0 <= q.iterations <= 64 and 1 <= q.levels <= 8 and
                0 < q.data_scale < INF):
            refuse("range", "bp_params")
        by["bp_ws_bytes"] = int(lib.smx_bp_workspace_bytes(w, h, size_d, q.levels, 2))
        if by["bp_ws_bytes"] == 0:
            refuse("shape", "aggregation")
        if by["bp_ws_bytes"] + 2 * size_d * n * 4 > max_ws_bytes:
            refuse("budget", "aggregation")
    o["so_params"] = buf["so_cost"] = buf["so_ws"] = buf["_so_chunk"] = None
    by["so_ws_bytes"] = 0
    if so:
        if s_begin != 0 or s_end != size_d:
            refuse("slices", "aggregation")
        o["so_params"] = scanline_params if scanline_params is not None else _lib.default_scanline_params()
        by["so_ws_bytes"] = int(lib.smx_scanline_workspace_bytes(w, h, size_d, 2))
        if by["so_ws_bytes"] == 0:
            refuse("shape", "aggregation")
        if by["so_ws_bytes"] + 2 * size_d * n * 4 > max_ws_bytes:
            refuse("budget", "aggregation")
        max_ws_bytes -= by["so_ws_bytes"] + 2 * size_d * n * 4      # what is left for the chain's cross stage
    local = max(1, s_end - s_begin)
    sif = local if slices_in_flight is None else max(1, min(local, int(slices_in_flight)))
    need = (lambda k: lib.smx_agg_workspace_bytes(w, h, k)) if multi_kernel else \
           (lambda k: lib.smx_agg_workspace_bytes_for(C.byref(params), w, h, k))
    o["guidance"] = guidance
    buf["cgf_ws"] = buf["cgf_cost"] = None
    by["cgf_ws_bytes"] = 0
    if guidance:
        if lib.smx_cgf_workspace_bytes(w, h, 1, 2) == 0:
            refuse("shape", "guidance")
        need = lambda k: (lib.smx_cgf_workspace_bytes(w, h, k, 2) + (0 if cost else 2 * k * n * 4)) // 2
    o["cross_params"] = buf["cross_ws"] = buf["cross_cost"] = None
    by["cross_ws_bytes"] = 0
    if cross:
        o["cross_params"] = cross_params if cross_params is not None else _lib.default_cross_params()
        if lib.smx_cross_workspace_bytes(w, h, 1, 2) == 0:
            refuse("shape", "aggregation")
        need = lambda k: (lib.smx_cross_workspace_bytes(w, h, k, 2) + (0 if cost else 2 * k * n * 4) +
                          (2 * k * n * 4 if so and k < local else 0)) // 2
    o["cost"] = cost
    o["adcensus_params"] = buf["adcensus_table"] = None
    if cost == "adcensus":
        o["adcensus_params"] = adcensus_params if adcensus_params is not None else _lib.default_adcensus_params()
        o["census_params"] = o["adcensus_params"].census
    elif cost == "mi":
        o["census_params"] = None
    else:
        o["census_params"] = (census_params if census_params is not None else _lib.default_census_params()) if cost else None
    o["mi_params"] = buf["mi_hist"] = buf["mi_table"] = None
    if cost == "mi":
        o["mi_params"] = mi_params if mi_params is not None else _lib.default_mi_params()
        if not (1 <= o["mi_params"].iterations <= 16 and o["mi_params"].init in _lib.MI_INITS.values()):
            refuse("range", "mi_params")
    chunk_cost = (lambda k: 2 * k * n * 4) if cost else (lambda k: 0)
    while sif > 1 and 2 * need(sif) + chunk_cost(sif) > max_ws_bytes:
        sif = (sif + 1) // 2
    if so and cross and 2 * need(sif) + chunk_cost(sif) > max_ws_bytes:
        refuse("budget", "aggregation")
    o["slices_in_flight"] = sif
    by["ws_bytes"] = 0 if aggregation or guidance else 2 * int(need(sif))
    buf["ws"] = ((by["ws_bytes"],), U8, False)
    buf["keys"] = ((2, h, w), I64, False)
    buf["best"] = ((2, h, w), F32, False)
    buf["dmap"] = ((2, h, w), F32, False)
    buf["mean"] = ((2, h, w), U8, bool(aggregation or guidance))
    buf["occlusion"] = ((h, w), F32, False)
    buf["filled"] = ((h, w), F32, False)
    buf["agg"] = ((2, local, h, w), F32, False) if want_agg else None
    o["wmf"] = wmf
    o["wmf_params"] = (wmf_params if wmf_params is not None else _lib.default_wmf_params()) if wmf else None
    buf["refined"] = ((h, w), F32, False) if wmf else None
    o["subpixel"] = subpixel
    buf["nbr"] = ((2, 3, h, w), F32, False) if subpixel else None
    buf["sub"] = ((2, h, w), F32, False) if subpixel else None
    buf["sub_filled"] = ((h, w), F32, False) if subpixel else None
    o["uniqueness"] = uniqueness
    buf["uq"] = ((2, 3, h, w), F32, False) if uniqueness else None
    buf["unique"] = ((h, w), F32, False) if uniqueness else None
    buf["margin"] = ((h, w), F32, False) if uniqueness else None
    o["speckle"] = _lib.default_speckle_params() if speckle is True else speckle
    buf["despeckled"] = ((h, w), F32, False) if o["speckle"] else None
    by["speckle_ws_bytes"] = int(lib.smx_speckle_workspace_bytes(w, h)) if o["speckle"] else 0
    buf["speckle_ws"] = ((by["speckle_ws_bytes"],), U8, False) if o["speckle"] else None
    o["vote"] = _lib.default_vote_params() if vote is True else vote
    o["vote_arms"] = buf["voted"] = buf["vote_arms_plane"] = buf["vote_ws"] = None
    by["vote_ws_bytes"] = 0
    if o["vote"]:
        o["vote_arms"] = _lib.CrossParams.from_buffer_copy(vote_arms) if vote_arms is not None else _lib.default_cross_params()
        o["vote_arms"].iterations = 1
        by["vote_ws_bytes"] = int(lib.smx_vote_workspace_bytes(w, h))
        if by["vote_ws_bytes"] == 0 or not 1 <= size_d <= 512:
            refuse("shape", "vote")
        buf["voted"] = ((h, w), F32, False)
        buf["vote_arms_plane"] = ((h, w), I32, False)
        buf["vote_ws"] = ((by["vote_ws_bytes"],), U8, False)
    if o["adjust"]:
        buf["adjusted"] = ((h, w), F32, False)
        buf["adjust_ws"] = ((by["adjust_ws_bytes"],), U8, False)
    buf["codes"] = ((2, h, w), I64, False) if cost in ("census", "adcensus") else None
    if cost == "mi":
        buf["mi_hist"] = ((_lib.MI_LEVELS, _lib.MI_LEVELS), I32, False)
        buf["mi_table"] = ((_lib.MI_LEVELS, _lib.MI_LEVELS), U8, False)
    buf["census_cost"] = ((2, sif, h, w), F32, False) if cost and not sgm and not bp and aggregation != "scanline" else None
    if cost == "adcensus":
        buf["adcensus_table"] = ((_lib.ADCENSUS_TABLE_FLOATS,), F32, False)
    if sgm:
        buf["sgm_cost"] = ((2, size_d, h, w), F32, False)
        buf["sgm_ws"] = ((by["sgm_ws_bytes"],), U8, False)
    if bp:
        buf["bp_cost"] = ((2, size_d, h, w), F32, False)
        buf["bp_ws"] = ((by["bp_ws_bytes"],), U8, False)
    if so:
        buf["so_cost"] = ((2, size_d, h, w), F32, False)
        buf["so_ws"] = ((by["so_ws_bytes"],), U8, False)
        buf["_so_chunk"] = ((2, sif, h, w), F32, False) if cross and sif < local else None
    if guidance:
        by["cgf_ws_bytes"] = int(lib.smx_cgf_workspace_bytes(w, h, sif, 2))
        buf["cgf_ws"] = ((by["cgf_ws_bytes"],), U8, False)
        buf["cgf_cost"] = None if cost else ((2, sif, h, w), F32, False)
    if cross:
        by["cross_ws_bytes"] = int(lib.smx_cross_workspace_bytes(w, h, sif, 2))
        buf["cross_ws"] = ((by["cross_ws_bytes"],), U8, False)
        buf["cross_cost"] = None if cost else ((2, sif, h, w), F32, False)
    o["pm_params"] = buf["pm_planes"] = buf["pm_disp"] = buf["pm_ws"] = None
    by["pm_ws_bytes"] = 0
    if pm:
        o["pm_params"] = pm_params if pm_params is not None else _lib.default_pm_params()
        by["pm_ws_bytes"] = int(lib.smx_pm_workspace_bytes(w, h))
        if by["pm_ws_bytes"] == 0 or not (1 <= size_d <= 1 << 20 and abs(dminl) <= 1 << 20 and abs(dminr) <= 1 << 20):
            refuse("shape", "aggregation")
        if by["pm_ws_bytes"] + 8 * n * 4 > max_ws_bytes:
            refuse("budget", "aggregation")
        buf["pm_planes"] = ((2, 3, h, w), F32, False)
        buf["pm_disp"] = ((2, h, w), F32, False)
        buf["pm_ws"] = ((by["pm_ws_bytes"],), U8, False)
        buf["sub_filled"] = ((h, w), F32, False)
    o["permeability"] = _lib.default_perm_params() if permeability is True else permeability
    buf["perm_ws"], by["perm_ws_bytes"] = None, 0
    if o["permeability"]:
        if lib.smx_perm_workspace_bytes(w, h, size_d, 2) == 0:
            refuse("shape", "permeability")
        per = 2 * n * 4
        by["perm_ws_bytes"] = per * (2 + min(size_d, max(1, (1 << 30) // per - 2)))
        buf["perm_ws"] = ((by["perm_ws_bytes"],), U8, False)
    o["cross_scale"] = _lib.default_cscale_params() if cross_scale is True else cross_scale
    levels, buf["cs_gray"], buf["cs_rgb"] = [], [], []
    if o["cross_scale"]:
        colour = bool(guidance) or (cost == "adcensus" and bool(o["adcensus_params"].colour))
        for s in range(1, o["cross_scale"].scales):
            ws, hs, dl, sl = cscale_level(lib, w, h, dminl, size_d, s)
            _, _, dr, sr = cscale_level(lib, w, h, dminr, size_d, s)
            if ws < 2:
                refuse("level", "cross_scale")
                break                       # (the constructor stopped here)
            handed = dict(w=ws, h=hs, size_d=max(sl, sr), dminl=dl, dminr=dr, want_agg=True, params=params,
                          max_ws_bytes=max_ws_bytes, multi_kernel=multi_kernel, cost=cost, census_params=census_params,
                          guidance=guidance, adcensus_params=adcensus_params)
            verdict, level = pipeline(lib, **handed)
            if verdict == "refused":
                R.extend((keywords, "level:" + kind) for keywords, kind in level)
                break
            # (the levels take the table of level 0: the constructor replaces the level's own mi_table by its own)
            levels.append(dict(handed=handed, shares=("mi_table",), outcome=level))
            buf["cs_gray"].append(((2, hs, ws), U8, False))
            buf["cs_rgb"].append(((2 * hs * ws * 4,), U8, False) if colour else None)
    buf["_agg_chunk"] = ((2, sif, h, w), F32, False) \
        if (cost or guidance or cross) and want_agg and sif < local and not sgm and not bp and not so else None
    if R:
        return "refused", R
    return "ok", dict(options=o, bytes=by, buffers=buf, levels=levels)


def cscale_level(lib, w, h, dmin, size_d, s):
    """_lib.cscale_level on the given library."""
    out = [C.c_int() for _ in range(4)]
    assert lib.smx_cscale_level(int(w), int(h), int(dmin), int(size_d), int(s), *[C.byref(v) for v in out]) == 0
    return tuple(v.value for v in out)


def shard_range(size_d, rank, world):
    return (rank * size_d) // world, ((rank + 1) * size_d) // world


def sharded(lib, w, h, size_d, rank=0, world=1, **kw):
    """ShardedPair.__init__: its own refusals, then the pipeline's on this rank's slice range.  -> as pipeline()."""
    R = []

    def refuse(kind, *keywords):
        R.append((keywords, kind))

    if world > 1 and kw.get("subpixel") is not None:
        refuse("world", "subpixel")
    if kw.get("cost") is not None:
        refuse("sharded", "cost")
    if kw.get("speckle") is not None:
        refuse("sharded", "speckle")
    if kw.get("vote") is not None or kw.get("vote_arms") is not None:
        refuse("sharded", "vote")
    if kw.get("adjust") is not None:
        refuse("sharded", "adjust")
    if kw.get("permeability") is not None:
        refuse("sharded", "permeability")
    if kw.get("cross_scale") is not None:
        refuse("sharded", "cross_scale")
    if kw.get("aggregation") in ("scanline", "cross-scanline") or kw.get("scanline_params") is not None:
        refuse("sharded", "aggregation")
    if kw.get("aggregation") == "patchmatch" or kw.get("pm_params") is not None:
        refuse("sharded", "aggregation")
    if kw.get("aggregation") == "bp" or kw.get("bp_params") is not None:
        refuse("sharded", "aggregation")
    if kw.get("aggregation") is not None:
        refuse("sharded", "aggregation")     # (whatever the value, under the name of semi-global matching)
    s0, s1 = shard_range(size_d, rank, world)
    verdict, out = pipeline(lib, w, h, size_d, s_begin=s0, s_end=s1, **kw)
    if R or verdict == "refused":
        return "refused", R + (out if verdict == "refused" else [])
    return "ok", out
