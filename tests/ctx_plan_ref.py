"""What the persistent context refuses and plans for a pair, as the context stated it before it had a stage table.

This is the refusal chain of ctx_pair, its PairNeeds initialiser, its walker-status list and the refusal list of
smx_ctx_stereo_pair_async, transcribed statement for statement from csrc/smx_ctx.hip as of commit 64e2533 ("Add hierarchical
belief propagation as an opt-in aggregation"), in the order of that file.  It is the reference of tests/test_ctx_plan_cpu.py
and is not derived from csrc/smx_ctx_plan.h: a rule that moves there shows as a difference here.

Every setting is a bool (or an array of bools: the operators are & | ~, so one call decides a whole grid of settings).  Where
the C++ returned at a refusal, `Chain.refuse` records it and goes on, so that a point keeps every refusal that applies to it,
in the order of the chain; the verdict is "some refusal applies", and the first one is what the old code reported.
"""
import numpy as np

SMX_SGM_MAX_D = 256
SMX_BP_MAX_D = 256
ADJ_MAX_D = 512
CGF_MAX_H = 65535

# the setter that switches each setting on
SETTERS = {
    "census": "smx_ctx_set_cost", "adcensus": "smx_ctx_set_adcensus", "sgm": "smx_ctx_set_aggregation", "cgf": "smx_ctx_set_guidance",
    "cross": "smx_ctx_set_cross", "so": "smx_ctx_set_scanline", "cscale": "smx_ctx_set_cross_scale", "perm": "smx_ctx_set_permeability",
    "bp": "smx_ctx_set_bp", "pm": "smx_ctx_set_patchmatch", "adjust": "smx_ctx_set_adjust", "uniq": "smx_ctx_set_uniqueness",
    "subpix": "smx_ctx_set_subpixel", "speckle": "smx_ctx_set_speckle", "vote": "smx_ctx_set_vote",
}
# the members of PairNeeds, in the order of the struct
NEEDS = ("cost", "agg", "subpix", "census", "sgm", "speckle", "uniq", "cgf", "cross", "vote", "so", "adjust", "cscale", "level",
         "pm", "perm", "bp")


def _wh_ok(w, h):
    return w >= 1 and h >= 1 and w * h < (1 << 31)


def sgm_shape_ok(w, h, size_d):                 # smx_capi.hip (the scan-line optimiser and belief propagation use it too)
    return _wh_ok(w, h) and 1 <= size_d <= SMX_SGM_MAX_D


def cross_shape_ok(w, h):                       # smx_cross.hip
    return _wh_ok(w, h)


def adjust_shape_ok(w, h, size_d):              # smx_adjust.hip
    return _wh_ok(w, h) and 1 <= size_d <= ADJ_MAX_D


def cscale_shape_ok(w, h, size_d):              # smx_cscale.hip
    return _wh_ok(w, h) and 1 <= size_d <= (1 << 20)


def perm_shape_ok(w, h, size_d):                # smx_perm.hip
    return _wh_ok(w, h) and 1 <= size_d <= (1 << 20)


def pm_shape_ok(w, h, size_d, dminl, dminr):    # smx_patchmatch.hip
    lim = 1 << 20
    return _wh_ok(w, h) and w < (1 << 24) and 1 <= size_d <= lim and -lim <= dminl <= lim and -lim <= dminr <= lim


def cgf_takes(w, h):                            # smx_cgf_workspace_bytes(w, h, 1, 2) != 0: cgf_shape_ok of smx_capi.hip
    return _wh_ok(w, h) and h <= CGF_MAX_H


class Chain:
    """The refusals of one walk down the chain: (where it applies, its kind, the settings it is about)."""

    def __init__(self):
        self.refusals = []

    def refuse(self, cond, kind, *stages):
        self.refusals.append((np.asarray(cond, bool), kind, stages))

    def refused(self):
        out = False
        for cond, _, _ in self.refusals:
            out = out | cond
        return np.asarray(out, bool)

    def count(self):
        return sum(cond.astype(np.int32) for cond, _, _ in self.refusals)


def pair(s, w, h, size_d, channels, dminl, dminr, wants_cost, wants_agg, wants_mean):
    """ctx_pair between its in-flight check and ctx_reserve.  s: the settings by the names of SETTERS plus "adc_colour";
    channels: 0 on the gray entry.  -> (the Chain, the PairNeeds as a dict, "the pair reads the walker's status word")."""
    c = Chain()
    mean = wants_mean
    rgb_entry = bool(channels)
    sgm, cgf = s["sgm"], s["cgf"]
    c.refuse(sgm & mean, "mean", "sgm")
    c.refuse(cgf & (not rgb_entry), "entry", "cgf")
    c.refuse(cgf & sgm, "conflict", "cgf", "sgm")
    c.refuse(cgf & mean, "mean", "cgf")
    c.refuse(cgf & (not cgf_takes(w, h)), "shape", "cgf")
    cross = s["cross"]
    c.refuse(cross & sgm, "conflict", "cross", "sgm")
    c.refuse(cross & cgf, "conflict", "cross", "cgf")
    c.refuse(cross & mean, "mean", "cross")
    c.refuse(cross & (not cross_shape_ok(w, h)), "shape", "cross")
    so = s["so"]
    c.refuse(so & sgm, "conflict", "so", "sgm")
    c.refuse(so & cgf, "conflict", "so", "cgf")
    c.refuse(so & mean, "mean", "so")
    c.refuse(so & (not sgm_shape_ok(w, h, size_d)), "shape", "so")
    c.refuse(s["adcensus"] & s["adc_colour"] & (not rgb_entry), "entry", "adcensus")
    adjust = s["adjust"]
    c.refuse(adjust & (not adjust_shape_ok(w, h, size_d)), "shape", "adjust")
    cscale = s["cscale"]
    # (one refusal that names the first of sgm, so, cross; recorded per partner)
    for other in ("sgm", "so", "cross"):
        c.refuse(cscale & s[other], "conflict", "cscale", other)
    c.refuse(cscale & mean, "mean", "cscale")
    c.refuse(cscale & (not cscale_shape_ok(w, h, size_d)), "shape", "cscale")
    perm = s["perm"]
    for other in ("sgm", "so", "cross"):
        c.refuse(perm & s[other], "conflict", "perm", other)
    c.refuse(perm & cscale, "conflict", "perm", "cscale")
    c.refuse(perm & mean, "mean", "perm")
    c.refuse(perm & (not perm_shape_ok(w, h, size_d)), "shape", "perm")
    bp, pm = s["bp"], s["pm"]
    # if (bp) { the `with` ladder; the mean images; the shape }
    for other in ("sgm", "cgf", "cross", "so", "cscale", "perm", "pm"):
        c.refuse(bp & s[other], "conflict", "bp", other)
    c.refuse(bp & mean, "mean", "bp")
    c.refuse(bp & (not sgm_shape_ok(w, h, size_d)), "shape", "bp")
    # if (pm) { the `with` ladder; the volumes and the mean images; the shape }
    for other in ("census", "adcensus", "cgf", "sgm", "cross", "so", "cscale", "perm", "adjust", "uniq", "subpix"):
        c.refuse(pm & s[other], "conflict", "pm", other)
    c.refuse(pm & (wants_cost | wants_agg | mean), "pm_out", "pm")
    c.refuse(pm & (not pm_shape_ok(w, h, size_d, dminl, dminr)), "shape", "pm")
    # const PairNeeds need = {...}
    false = np.zeros(np.shape(sgm), bool)
    need = {
        "cost": wants_cost | sgm | bp | (so & ~cross),
        "agg": wants_agg | adjust | cscale | perm,
        "subpix": s["subpix"],
        "census": s["census"] | s["adcensus"],
        "sgm": sgm, "speckle": s["speckle"], "uniq": s["uniq"], "cgf": cgf, "cross": cross, "vote": s["vote"], "so": so,
        "adjust": adjust, "cscale": cscale, "level": false, "pm": pm, "perm": perm, "bp": bp,
    }
    need = {k: np.asarray(v, bool) | false for k, v in need.items()}
    # if (!need.sgm && !need.bp && !need.cgf && !need.cross && !need.so && !need.pm) smx_dev_agg_status(...)
    walker = ~need["sgm"] & ~need["bp"] & ~need["cgf"] & ~need["cross"] & ~need["so"] & ~need["pm"]
    return c, need, walker


# smx_ctx_stereo_pair_async: the settings it refuses, in the order of its list, and the entry each message points to
ASYNC_ORDER = ("subpix", "speckle", "vote", "adjust", "cscale", "perm", "bp", "pm", "uniq", "sgm", "cgf", "cross", "so", "census",
               "adcensus")
ASYNC_USE = {k: "smx_ctx_stereo_pair_rgb" if k == "cgf" else "smx_ctx_stereo_pair" for k in ASYNC_ORDER}


def pair_async(s):
    """-> the Chain of smx_ctx_stereo_pair_async; an accepted pair needs PairNeeds{} and reads the walker's status word."""
    c = Chain()
    for k in ASYNC_ORDER:
        c.refuse(s[k], "async", k)
    return c
