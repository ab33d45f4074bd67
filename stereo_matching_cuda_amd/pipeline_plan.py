"""What a PairPipeline refuses, owns and sizes: one table of the opt-in stages and one function that plans a pipeline from it.

Host arithmetic only: no torch, no device.  STAGES has a row per opt-in; plan_pipeline() checks a
constructor call against the rows and returns a PipelinePlan -- the options with their defaults applied, `slices_in_flight`,
every byte count, and the buffers as (attribute, shape, dtype, zeroed) -- which PairPipeline allocates in one loop and
ShardedPair reads the "sharded" column of.  The workspace sizes come from the library's host queries (smx_*_workspace_bytes),
on the handle that is passed in.
"""
import ctypes as C
from dataclasses import dataclass, field
from types import SimpleNamespace

from . import _lib

INF = float("inf")
U8, I32, I64, F32 = "uint8", "int32", "int64", "float32"


@dataclass(frozen=True)
class Stage:
    """One opt-in.  It is on where `kw` has one of `values` (a keyword of named choices), is not None (a keyword that takes
    None, True or `struct`; a number), or is true (`flag`)."""
    key: str                    # the row's name
    kw: str                     # the constructor keyword that switches it on
    noun: str                   # what the messages call it
    values: tuple = ()          # the values of `kw` that are this row
    struct: type = None         # the struct `kw` takes beside None and True
    flag: bool = False          # `kw` is a plain switch
    default: object = None      # factory of the default of the struct, or of `params_kw`
    params_kw: str = None       # the *_params keyword that belongs to the row ...
    params_attr: str = None     # ... the attribute the pipeline keeps it under (None: the keyword itself) ...
    params_type: type = None    # ... the type it is held to (None: not checked) ...
    strict: bool = False        # ... and whether it is refused where the row is off
    range_ok: object = None     # predicate of the parameters ...
    range_text: str = None      # ... and the sentence that states it
    whole: str = None           # why it needs the whole slice range (None: a slice sub-range is fine)
    ws: object = None           # (library, geometry, slices) -> the bytes of its workspace; 0: it does not take the shape
    max_d: int = None           # the most labels it takes
    max_dmin: int = None        # the largest |dminl|, |dminr| it takes
    limit: str = None           # the sentence of its shape limit
    holds: object = None        # geometry -> the bytes it holds beside its workspace that max_ws_bytes counts ...
    holds_text: str = None      # ... what they are ...
    deducts: bool = False       # ... and whether they are taken off what the aggregation behind it may use
    forces_agg: bool = False    # the aggregation keeps its volumes in self.agg as with want_agg
    no_walker: bool = False     # the pipeline has no mean images (self.mean stays zero) and no fused-walker workspace
    sharded: bool = False       # the sharded driver takes it
    owns: object = None         # plan in progress -> [(attribute, shape, dtype)]: the buffers it brings


def _volumes(g):
    return 2 * g.size_d * g.n * 4           # two whole volumes of floats


def _plane(g, *lead):
    return lead + (g.h, g.w)


def _whole_stage(prefix):
    """The buffers of an aggregation that reads both whole cost volumes."""
    return lambda p: [(prefix + "_cost", _plane(p, 2, p.size_d), F32), (prefix + "_ws", (p.bytes[prefix + "_ws_bytes"],), U8)]


def _chunk_stage(prefix):
    """The buffers of an aggregation that runs over chunks of `slices_in_flight` slices: its workspace, and the chunk's cost
    slices where the cost is the reference's (the other costs have self.census_cost)."""
    return lambda p: [(prefix + "_ws", (p.bytes[prefix + "_ws_bytes"],), U8)] + \
        ([] if p.cost else [(prefix + "_cost", _plane(p, 2, p.sif), F32)])


_WHOLE = "needs a pixel's whole disparity range"
_SGM_LIMIT = "w*h < 2^31, size_d <= 256"
_cross_ws = lambda L, g, n: L.smx_cross_workspace_bytes(g.w, g.h, n, 2)
_so_ws = lambda L, g, n: L.smx_scanline_workspace_bytes(g.w, g.h, g.size_d, 2)

# The rows, in the order in which they are charged against max_ws_bytes.
STAGES = (
    Stage("census", "cost", "the census cost", values=("census",), default=_lib.default_census_params, params_kw="census_params",
          owns=lambda p: [("codes", _plane(p, 2), I64)]),
    Stage("adcensus", "cost", "the AD-Census cost", values=("adcensus",), default=_lib.default_adcensus_params,
          params_kw="adcensus_params",
          owns=lambda p: [("codes", _plane(p, 2), I64), ("adcensus_table", (_lib.ADCENSUS_TABLE_FLOATS,), F32)]),
    Stage("mi", "cost", "the mutual-information cost", values=("mi",), default=_lib.default_mi_params, params_kw="mi_params",
          strict=True, range_ok=lambda q: 1 <= q.iterations <= 16 and q.init in _lib.MI_INITS.values(),
          range_text="1 <= iterations <= 16 and init 0 (random) or 1 (reference)",
          whole="learns its table from a pair's whole disparity range",
          owns=lambda p: [("mi_hist", (_lib.MI_LEVELS, _lib.MI_LEVELS), I32), ("mi_table", (_lib.MI_LEVELS, _lib.MI_LEVELS), U8)]),
    Stage("rgb", "guidance", "the colour-guided filter", values=("rgb",), ws=lambda L, g, n: L.smx_cgf_workspace_bytes(g.w, g.h, n, 2),
          limit="h <= 65535, w*h < 2^31", no_walker=True, sharded=True, owns=_chunk_stage("cgf")),
    Stage("adjust", "adjust", "the depth-discontinuity adjustment", struct=_lib.AdjustParams, default=_lib.default_adjust_params,
          range_ok=lambda q: 1 <= q.tau_e <= 512 and q.vertical in (0, 1) and 1 <= q.iterations <= 8,
          range_text="1 <= tau_e <= 512, vertical 0 or 1 and 1 <= iterations <= 8",
          whole="reads a pixel's whole aggregated column", ws=lambda L, g, n: L.smx_adjust_workspace_bytes(g.w, g.h), max_d=512,
          limit="w*h < 2^31, 1 .. 512 labels", holds=_volumes, holds_text="the two aggregated volumes and its workspace",
          deducts=True, forces_agg=True,
          owns=lambda p: [("adjusted", _plane(p), F32), ("adjust_ws", (p.bytes["adjust_ws_bytes"],), U8)]),
    Stage("sgm", "aggregation", "semi-global matching", values=("sgm",), default=_lib.default_sgm_params, params_kw="sgm_params",
          whole=_WHOLE, ws=lambda L, g, n: L.smx_sgm_workspace_bytes(g.w, g.h, g.size_d, 2), limit=_SGM_LIMIT, holds=_volumes,
          holds_text="its workspace and the two whole cost volumes", no_walker=True, owns=_whole_stage("sgm")),
    Stage("bp", "aggregation", "belief propagation", values=("bp",), default=_lib.default_bp_params, params_kw="bp_params",
          strict=True,
          range_ok=lambda q: (0 <= q.step <= 4095 and 0 <= q.trunc <= 4095 and 0 <= q.iterations <= 64 and 1 <= q.levels <= 8 and
                              0 < q.data_scale < INF),
          range_text="0 <= step, trunc <= 4095, 0 <= iterations <= 64, 1 <= levels <= 8 and a finite data_scale > 0",
          whole=_WHOLE, ws=lambda L, g, n: L.smx_bp_workspace_bytes(g.w, g.h, g.size_d, g.bp_params.levels, 2), limit=_SGM_LIMIT,
          holds=_volumes, holds_text="its workspace and the two whole cost volumes", no_walker=True, owns=_whole_stage("bp")),
    Stage("cross", "aggregation", "cross-based aggregation", values=("cross",), default=_lib.default_cross_params,
          params_kw="cross_params", ws=_cross_ws, limit="w*h < 2^31", no_walker=True, owns=_chunk_stage("cross")),
    Stage("scanline", "aggregation", "the scan-line optimiser", values=("scanline",), default=_lib.default_scanline_params,
          params_kw="scanline_params", params_attr="so_params", strict=True, whole=_WHOLE, ws=_so_ws, limit=_SGM_LIMIT, holds=_volumes,
          holds_text="its workspace and the two whole cost volumes", deducts=True, no_walker=True, owns=_whole_stage("so")),
    # (Mei's chain: the cross stage's row for its chunks -- cross_params, self.cross_ws -- and the optimiser's for the rest; what
    # the optimiser holds is taken off what the cross stage may use)
    Stage("cross-scanline", "aggregation", "the chain of cross-based aggregation and the scan-line optimiser",
          values=("cross-scanline",), default=_lib.default_scanline_params, params_kw="scanline_params", params_attr="so_params",
          strict=True, whole=_WHOLE, ws=_so_ws, limit=_SGM_LIMIT, holds=_volumes,
          holds_text="its workspace and the two whole cost volumes", deducts=True, no_walker=True,
          owns=lambda p: _whole_stage("so")(p) + _chunk_stage("cross")(p) +
          ([("_so_chunk", _plane(p, 2, p.sif), F32)] if p.sif < p.local else [])),
    Stage("patchmatch", "aggregation", "PatchMatch stereo", values=("patchmatch",), default=_lib.default_pm_params,
          params_kw="pm_params", params_type=_lib.PMParams, strict=True,
          range_ok=lambda q: 0 <= q.radius <= 17 and 0.0 < q.gamma < INF and 1 <= q.iterations <= 16 and 0.0 <= q.max_slope <= 8.0,
          range_text="0 <= radius <= 17, a finite gamma > 0, 1 <= iterations <= 16 and 0 <= max_slope <= 8",
          whole="searches a pixel's whole disparity range", ws=lambda L, g, n: L.smx_pm_workspace_bytes(g.w, g.h), max_d=1 << 20,
          max_dmin=1 << 20, limit="w < 2^24, w*h < 2^31, size_d and |dmin| <= 2^20", holds=lambda g: 8 * g.n * 4,
          holds_text="its planes and workspace", no_walker=True,
          owns=lambda p: [("pm_planes", _plane(p, 2, 3), F32), ("pm_disp", _plane(p, 2), F32), ("pm_ws", (p.bytes["pm_ws_bytes"],), U8),
                          ("sub_filled", _plane(p), F32)]),
    Stage("cross_scale", "cross_scale", "cross-scale aggregation", struct=_lib.CScaleParams, default=_lib.default_cscale_params,
          range_ok=lambda q: 1 <= q.scales <= 5 and 0.0 <= q.lambda_ < INF, range_text="1 <= scales <= 5 and a finite lambda >= 0",
          whole="combines whole volumes", forces_agg=True),
    # (its workspace, at most ~1 GiB, is deliberately not counted in max_ws_bytes)
    Stage("permeability", "permeability", "the permeability filter", struct=_lib.PermParams, default=_lib.default_perm_params,
          range_ok=lambda q: 0.0 < q.sigma < INF, range_text="a finite sigma > 0", whole="runs over whole volumes",
          ws=lambda L, g, n: L.smx_perm_workspace_bytes(g.w, g.h, g.size_d, 2), limit="w*h < 2^31, size_d <= 2^20", forces_agg=True,
          owns=lambda p: [("perm_ws", (p.bytes["perm_ws_bytes"],), U8)]),
    # (the state belongs to the keys of ONE volume: after a key reduction across D-shards it would be tested against winners it
    # does not belong to)
    Stage("uniqueness", "uniqueness", "the uniqueness test", whole="keeps a state that does not combine across D-shards",
          sharded=True, owns=lambda p: [("uq", _plane(p, 2, 3), F32), ("unique", _plane(p), F32), ("margin", _plane(p), F32)]),
    Stage("subpixel", "subpixel", "the sub-pixel fit", values=tuple(_lib.SUBPIX_MODES), sharded=True,
          owns=lambda p: [("nbr", _plane(p, 2, 3), F32), ("sub", _plane(p, 2), F32), ("sub_filled", _plane(p), F32)]),
    Stage("speckle", "speckle", "speckle removal", struct=_lib.SpeckleParams, default=_lib.default_speckle_params,
          ws=lambda L, g, n: L.smx_speckle_workspace_bytes(g.w, g.h),
          owns=lambda p: [("despeckled", _plane(p), F32), ("speckle_ws", (p.bytes["speckle_ws_bytes"],), U8)]),
    Stage("vote", "vote", "region voting", struct=_lib.VoteParams, default=_lib.default_vote_params, params_kw="vote_arms",
          params_type=_lib.CrossParams, strict=True, ws=lambda L, g, n: L.smx_vote_workspace_bytes(g.w, g.h), max_d=512,
          limit="w*h < 2^31, size_d <= 512",
          owns=lambda p: [("voted", _plane(p), F32), ("vote_arms_plane", _plane(p), I32), ("vote_ws", (p.bytes["vote_ws_bytes"],), U8)]),
    Stage("wmf", "wmf", "the weighted-median refinement", values=("occluded", "all"), default=_lib.default_wmf_params,
          params_kw="wmf_params", sharded=True, owns=lambda p: [("refined", _plane(p), F32)]),
    Stage("want_agg", "want_agg", "the aggregated volumes", flag=True, forces_agg=True, sharded=True),
)
ROWS = {r.key: r for r in STAGES}
AGGREGATIONS = tuple(r.key for r in STAGES if r.kw == "aggregation")
COSTS = tuple(r.key for r in STAGES if r.kw == "cost")
CHUNKED = {"rgb": ("cgf", ROWS["rgb"].ws), "cross": ("cross", _cross_ws), "cross-scanline": ("cross", _cross_ws)}
# the byte count a row's workspace is kept under (the chain's cross workspace: CHUNKED)
WS_BYTES = {"adjust": "adjust_ws_bytes", "sgm": "sgm_ws_bytes", "bp": "bp_ws_bytes", "scanline": "so_ws_bytes",
            "cross-scanline": "so_ws_bytes", "patchmatch": "pm_ws_bytes", "speckle": "speckle_ws_bytes", "vote": "vote_ws_bytes"}

# What does not run together, each pair stated once: (rows, rows, why).  EXCLUDES is symmetric by construction.
_CONFLICTS = (
    (("rgb",), AGGREGATIONS, "colour guidance belongs to the guided filter"),
    (("cross_scale",), AGGREGATIONS, "cross-scale aggregation belongs to the guided filter (integer volumes and fixed penalties do "
                                      "not rescale across levels)"),
    (("permeability",), AGGREGATIONS, "the permeability filter runs behind the guided filter"),
    (("permeability",), ("cross_scale",), "the permeability filter is not built behind cross-scale aggregation"),
    (("patchmatch",), COSTS + ("adjust", "uniqueness", "subpixel", "want_agg"),
     "PatchMatch stereo keeps no cost volume and its planes are sub-pixel already"),
)
EXCLUDES = {r.key: {} for r in STAGES}
for _a, _b, _why in _CONFLICTS:
    for _x in _a:
        for _y in _b:
            EXCLUDES[_x][_y] = EXCLUDES[_y][_x] = _why

# every attribute of a pipeline that is a buffer or None (the levels' pyramids are the lists cs_gray, cs_rgb beside them)
BUFFERS = ("ws", "keys", "best", "dmap", "mean", "occlusion", "filled", "agg", "refined", "nbr", "sub", "sub_filled", "uq", "unique",
           "margin", "despeckled", "speckle_ws", "voted", "vote_arms_plane", "vote_ws", "adjusted", "adjust_ws", "codes", "mi_hist",
           "mi_table", "census_cost", "adcensus_table", "sgm_cost", "sgm_ws", "bp_cost", "bp_ws", "so_cost", "so_ws", "_so_chunk",
           "cgf_ws", "cgf_cost", "cross_ws", "cross_cost", "pm_planes", "pm_disp", "pm_ws", "perm_ws", "_agg_chunk")
# the plain arguments of the constructor: geometry, device, and the sizes the rows are planned within
GEOMETRY = ("w", "h", "size_d", "dminl", "dminr", "s_begin", "s_end", "device", "slices_in_flight", "params", "max_ws_bytes",
            "multi_kernel")
LEVEL_SHARES = ("mi_table",)        # what a cross-scale level takes from level 0 in place of its own


@dataclass
class PipelinePlan:
    options: dict               # attribute -> value: the geometry and every option with its default applied
    on: tuple                   # the keys of the rows that are on
    slices_in_flight: int
    bytes: dict                 # ws_bytes and every *_ws_bytes
    buffers: list               # (attribute, shape, dtype, zeroed)
    levels: list = field(default_factory=list)      # per cross-scale level: (what it was planned from, its plan, shape of cs_gray[i], of cs_rgb[i] or None)
    no_walker: bool = False     # no mean images, no fused-walker workspace, no status word to read


def is_on(row, value):
    return bool(value) if row.flag else value in row.values if row.values else value is not None


def _say(values):
    words = ["None"] + [repr(v) for v in values]
    return ", ".join(words[:-1]) + " or " + words[-1]


def stages_on(opt):
    """The rows a set of keywords switches on, after the check of each keyword's value."""
    for kw in dict.fromkeys(r.kw for r in STAGES):
        rows = [r for r in STAGES if r.kw == kw]
        v, row = opt.get(kw), rows[0]
        if row.flag or v is None:
            continue
        if row.values:
            accepted = [x for r in rows for x in r.values]
            if v not in accepted:
                raise ValueError(f"{kw} must be {_say(accepted)}, not {v!r}")
        elif row.struct:
            if v is not True and not isinstance(v, row.struct):
                raise ValueError(f"{kw} must be None, True or {row.struct.__name__}, not {v!r}")
        else:
            try:
                ok = 0.0 < float(v) < INF
            except ValueError:
                ok = False
            if not ok:
                raise ValueError(f"{kw} must be None or a finite ratio > 0, not {v!r}")
    return [r for r in STAGES if is_on(r, opt.get(r.kw))]


def _label(row, opt):
    return f"{row.noun} ({row.kw}={opt[row.kw]!r})" if row.values else f"{row.noun} ({row.kw}=)"


def plan_pipeline(lib, w, h, size_d, dminl=None, dminr=0, s_begin=0, s_end=None, slices_in_flight=None, params=None,
                  max_ws_bytes=64 << 30, multi_kernel=False, **opt):
    """The plan of PairPipeline(w, h, size_d, ..., **opt), or ValueError with the rule that refuses it.  Allocates nothing."""
    kws = {r.kw for r in STAGES} | {r.params_kw for r in STAGES if r.params_kw}
    for k in opt:
        if k not in kws:
            raise TypeError(f"plan_pipeline() got an unexpected keyword argument {k!r}")
    opt = {k: opt.get(k) for k in kws}
    on = stages_on(opt)
    keys = [r.key for r in on]
    g = SimpleNamespace(w=int(w), h=int(h), size_d=int(size_d), dminr=int(dminr), s_begin=int(s_begin))
    g.n = g.w * g.h
    g.dminl = -(g.size_d - 1) if dminl is None else int(dminl)
    g.s_end = g.size_d if s_end is None else int(s_end)
    g.params = params if params is not None else _lib.default_params()
    # the options as the pipeline keeps them: a keyword of choices as given, a struct or *_params with its default where its row
    # is on and None where it is off
    o = dict(vars(g))
    for r in STAGES:
        if not r.flag:
            o[r.kw] = None if r.struct else opt[r.kw]
        if r.params_kw:
            o[r.params_attr or r.params_kw] = None
    if opt["uniqueness"] is not None:
        o["uniqueness"] = float(opt["uniqueness"])
    for r in STAGES:
        given = opt[r.params_kw] if r.params_kw else None
        if given is not None and r.strict and not any(x.params_kw == r.params_kw for x in on):
            owners = " / ".join(f"{x.kw}={x.values[0]!r}" if x.values else f"{x.kw}=" for x in STAGES if x.params_kw == r.params_kw)
            raise ValueError(f"{r.params_kw} belongs to {owners}: {r.noun} is off")
        if given is not None and r.params_type and not isinstance(given, r.params_type):
            raise ValueError(f"{r.params_kw} must be None or {r.params_type.__name__}, not {given!r}")
    for r in on:
        if r.params_kw:
            q = o[r.params_attr or r.params_kw] = opt[r.params_kw] if opt[r.params_kw] is not None else r.default()
        if r.struct:
            q = o[r.kw] = r.default() if opt[r.kw] is True else opt[r.kw]
        if r.range_ok and not r.range_ok(q):
            raise ValueError(f"{r.noun} ({r.kw if r.struct else r.params_kw}=) needs {r.range_text}")
    cost, aggregation = o["cost"], o["aggregation"]
    if cost == "adcensus":
        o["census_params"] = o["adcensus_params"].census           # (the codes are those of its census part)
    if aggregation == "cross-scanline":
        o["cross_params"] = opt["cross_params"] if opt["cross_params"] is not None else _lib.default_cross_params()
    if "vote" in keys:
        o["vote_arms"] = _lib.CrossParams.from_buffer_copy(opt["vote_arms"]) if opt["vote_arms"] is not None else \
            _lib.default_cross_params()
        o["vote_arms"].iterations = 1                               # (not read by the arms)
    g.bp_params = o["bp_params"]
    # what does not run together, and what needs the whole slice range
    for i, a in enumerate(on):
        for b in on[i + 1:]:
            if b.key in EXCLUDES[a.key]:
                raise ValueError(f"{EXCLUDES[a.key][b.key]}: {_label(a, opt)} does not run with {_label(b, opt)}")
    for r in on:
        if r.whole and (g.s_begin != 0 or g.s_end != g.size_d):
            raise ValueError(f"{_label(r, opt)} {r.whole}: no slice sub-range")
    # the shapes the rows take, and their workspaces
    by = dict.fromkeys(["ws_bytes", "cgf_ws_bytes", "cross_ws_bytes", "perm_ws_bytes"] + list(WS_BYTES.values()), 0)
    for r in on:
        size = int(r.ws(lib, g, 1)) if r.ws else None
        if r.limit and (size == 0 or (r.max_d and not 1 <= g.size_d <= r.max_d) or
                        (r.max_dmin and not (abs(g.dminl) <= r.max_dmin and abs(g.dminr) <= r.max_dmin))):
            raise ValueError(f"{_label(r, opt)} does not take {g.w} x {g.h} x {g.size_d} from {g.dminl} / {g.dminr} ({r.limit})")
        if r.key in WS_BYTES:
            by[WS_BYTES[r.key]] = size
    # the budget: what each row holds is counted against max_ws_bytes, and a row that deducts leaves the rest to those behind it
    left = max_ws_bytes
    for r in on:
        if r.holds:
            held = by[WS_BYTES[r.key]] + r.holds(g)
            if held > left:
                raise ValueError(f"{_label(r, opt)} needs {held} bytes for {r.holds_text}: more than max_ws_bytes = {left}")
            if r.deducts:
                left -= held
    # the slices in flight: halved until the chunked aggregation's workspace and cost slices fit what is left.  The workspace
    # of the path these parameters run (smx_agg_workspace_bytes_for follows the library's choice: a fused walker, one plane per
    # slice in flight, or the multi-kernel path); a forced multi-kernel path (smx_set_agg_path(1)) needs the parameter-agnostic
    # bound.  Pair calls (both views per launch) need twice the single-view workspace.
    local = max(1, g.s_end - g.s_begin)
    sif = local if slices_in_flight is None else max(1, min(local, int(slices_in_flight)))
    chunked = next((CHUNKED[k] for k in keys if k in CHUNKED), None)
    chain = "cross-scanline" in keys
    slices = lambda k: 2 * k * g.n * 4                  # k slices of both views

    def walker(k):
        return int(lib.smx_agg_workspace_bytes(g.w, g.h, k) if multi_kernel else
                   lib.smx_agg_workspace_bytes_for(C.byref(g.params), g.w, g.h, k))

    def in_flight(k):
        if chunked is None:
            return 2 * walker(k) + (slices(k) if cost else 0)
        # both views in one workspace; the reference's cost goes through a chunk buffer like the other costs, and the chain
        # also holds a chunk of q on its way into the whole volumes
        ws = int(chunked[1](lib, g, k)) + (0 if cost else slices(k)) + (slices(k) if chain and k < local else 0)
        return 2 * (ws // 2) + (slices(k) if cost else 0)

    while sif > 1 and in_flight(sif) > left:
        sif = (sif + 1) // 2
    if chain and in_flight(sif) > left:
        raise ValueError(f"{_label(ROWS['cross-scanline'], opt)} does not fit max_ws_bytes = {max_ws_bytes}")
    o["slices_in_flight"] = sif
    no_walker = any(r.no_walker for r in on)
    by["ws_bytes"] = 0 if no_walker else 2 * walker(sif)
    if chunked:
        by[chunked[0] + "_ws_bytes"] = int(chunked[1](lib, g, sif))
    if "permeability" in keys:
        # both views: two weight planes and a scratch plane per slice in flight, every slice at once within ~1 GiB
        per = 2 * g.n * 4
        by["perm_ws_bytes"] = per * (2 + min(g.size_d, max(1, (1 << 30) // per - 2)))
    # the buffers
    want_agg = any(r.forces_agg for r in on)
    whole_volumes = any(k in keys for k in ("sgm", "bp", "scanline", "cross-scanline"))
    p = SimpleNamespace(**vars(g), sif=sif, local=local, cost=cost, bytes=by)
    # keys[0] = left view, keys[1] = right view: one buffer so the shard merge is ONE all-reduce
    bufs = [("ws", (by["ws_bytes"],), U8), ("keys", _plane(g, 2), I64), ("best", _plane(g, 2), F32), ("dmap", _plane(g, 2), F32),
            ("mean", _plane(g, 2), U8), ("occlusion", _plane(g), F32), ("filled", _plane(g), F32)]
    if want_agg:
        bufs.append(("agg", _plane(g, 2, local), F32))
    if cost and aggregation not in ("sgm", "bp", "scanline"):
        bufs.append(("census_cost", _plane(g, 2, sif), F32))
    for r in on:
        bufs += r.owns(p) if r.owns else []
    if (cost or chunked) and want_agg and sif < local and not whole_volumes:
        # a chunk's aggregated slices of both views, copied into self.agg (whose views are `local` slices apart)
        bufs.append(("_agg_chunk", _plane(g, 2, sif), F32))
    plan = PipelinePlan(options=o, on=tuple(keys), slices_in_flight=sif, bytes=by, no_walker=no_walker,
                        buffers=[b + (b[0] == "mean" and no_walker,) for b in bufs])
    # the cross-scale levels: the same cost, guide and params at the level's geometry, both views with the larger of the two
    # views' label counts, each within what max_ws_bytes leaves
    if "cross_scale" in keys:
        colour = "rgb" in keys or (cost == "adcensus" and bool(o["adcensus_params"].colour))
        for s in range(1, o["cross_scale"].scales):
            ws, hs, dl, sl = cscale_level(lib, g.w, g.h, g.dminl, g.size_d, s)
            _, _, dr, sr = cscale_level(lib, g.w, g.h, g.dminr, g.size_d, s)
            if ws < 2:
                raise ValueError(f"cross-scale level {s} of a {g.w} x {g.h} pair (cross_scale=) is narrower than 2 pixels")
            handed = dict(w=ws, h=hs, size_d=max(sl, sr), dminl=dl, dminr=dr, want_agg=True, params=g.params, max_ws_bytes=left,
                          multi_kernel=multi_kernel, cost=cost, census_params=opt["census_params"], guidance=opt["guidance"],
                          adcensus_params=opt["adcensus_params"])
            plan.levels.append((handed, plan_pipeline(lib, **handed), (2, hs, ws), (2 * hs * ws * 4,) if colour else None))
    return plan


def cscale_level(lib, w, h, dmin, size_d, s):
    """(w_s, h_s, dmin_s, size_d_s): the geometry of level s of a cross-scale pyramid (smx_cscale_level)."""
    out = [C.c_int() for _ in range(4)]
    _lib.check(lib.smx_cscale_level(w, h, dmin, size_d, s, *[C.byref(v) for v in out]))
    return tuple(v.value for v in out)


def sharded_refusal(world, opt):
    """What the sharded driver refuses of a PairPipeline's keywords: the message, or None.  A row that is not `sharded` is
    refused where its keyword switches it on."""
    if world > 1 and opt.get("subpixel") is not None:
        # the neighbours of a winner at a shard boundary were aggregated on another rank
        return "subpixel needs the whole slice range on one rank (world == 1)"
    for r in STAGES:
        v = opt.get(r.kw)
        if not r.sharded and v is not None and (v in r.values or not r.values):
            use = f"{r.kw}={r.values[0]!r}" if r.values else f"{r.kw}=..."
            return f"{r.noun} is not part of the sharded driver: use PairPipeline({use})"
    return None
