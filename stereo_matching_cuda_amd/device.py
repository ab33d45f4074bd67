"""Device-resident pair pipeline: HBM buffers and streams come from PyTorch (plumbing only), all
compute goes through the smx_dev_* C-ABI on torch's current HIP stream.

One PairPipeline per (shape, slice range) per GPU; nothing is allocated after construction, so a
step is a fixed sequence of kernel launches on one stream.
"""
import ctypes as C

import torch

from . import _lib
from .pipeline_plan import BUFFERS, LEVEL_SHARES, plan_pipeline


def _dp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class PairPipeline:
    """main.cu:65-155 for one stereo pair, optionally restricted to slices [s_begin, s_end) of
    both volumes (the D-shard of this rank).  Layout in HBM: gray images u8 [h][w]; per view packed
    WTA keys i64 [h][w]; best/dmap/occlusion/filled f32 [h][w]; workspace = image / guidance planes +
    per slice in flight one aggregated plane and the strip hand-off records (smx_agg_workspace_bytes).
    Every launch goes to the pipeline's own device (torch.cuda.device(self.device)) on that device's
    current stream, whatever device is current in the calling thread."""

    def __init__(self, w, h, size_d, dminl=None, dminr=0, s_begin=0, s_end=None, device="cuda:0",
                 slices_in_flight=None, want_agg=False, params=None, max_ws_bytes=64 << 30, multi_kernel=False,
                 wmf=None, wmf_params=None, subpixel=None, cost=None, census_params=None, speckle=None,
                 aggregation=None, sgm_params=None, bp_params=None, uniqueness=None, guidance=None, adcensus_params=None, mi_params=None, cross_params=None,
                 vote=None, vote_arms=None, scanline_params=None, adjust=None, cross_scale=None, pm_params=None,
                 permeability=None):
        """wmf: None, "occluded" or "all" -- the weighted-median refinement of the filled left map (not a stage of
        the reference; smx_dev_weighted_median behind the finish on the same stream, into self.refined): "occluded"
        filters the pixels the LR check invalidated, "all" every pixel.  With None nothing is allocated or launched.
        subpixel: None, "parabola" or "equiangular" -- sub-pixel maps from the winners' neighbouring aggregated costs (not
        a stage of the reference): the aggregation keeps them in self.nbr (2, 3, h, w) through the _nbr entries, and
        finish() runs smx_dev_subpixel_pair into self.sub (2, h, w) and self.sub_filled (h, w).  With None nothing is
        allocated or launched.
        cost: None or "census" -- the matching cost.  None is the reference's (built on the fly inside the aggregation,
        or passed to aggregate()); nothing is allocated or launched for it.  "census" is the census / Hamming cost
        (include/smx.h smx_dev_census, smx_dev_census_cost_pair; census_params: CensusParams, None = the defaults): the
        pipeline owns the codes self.codes (2, h, w) and a cost buffer self.census_cost of `slices_in_flight` slices per
        view, which the max_ws_bytes bound counts, and aggregate(gray_l, gray_r) runs cost chunk -> aggregation from
        that chunk over its slice range.  th_color / th_grad / alpha of `params` are unused then.
        cost="adcensus" is AD-Census, census plus absolute differences (include/smx.h smx_dev_adcensus_cost_pair;
        adcensus_params: AdCensusParams, None = the defaults): the flows and buffers of the census cost, with the device table
        self.adcensus_table, uploaded here, beside them.  With adcensus_params.colour 1 the AD term comes from the colour
        images: aggregate() / run() need rgb_l=, rgb_r= then, with either guide.
        cost="mi" is the mutual-information cost (include/smx.h smx_dev_mi_cost_pair, smx_ctx_set_mi; mi_params: MiParams, None =
        the defaults): the flows and the cost buffer of the census cost without the codes, with self.mi_hist and self.mi_table
        (256, 256) beside them.  run() learns the table from the pair: the start map (random, or one pass with the reference's
        cost), then mi_params.iterations times histogram -> table on the host -> pass, the passes before the last stopping behind
        the LR check; aggregate() alone is one pass with the table that self.mi_table holds.  A host round trip per table:
        run() is not graph-capturable.  No slice sub-range, no PatchMatch stereo.
        speckle: None, True (the defaults) or SpeckleParams -- speckle removal (not a stage of the reference;
        smx_dev_speckle_filter behind the finish): self.despeckled = self.occlusion without its small connected components
        (vmin = dminl, new_val = dminl - 100), self.filled = the fill of self.despeckled, and the sub-pixel fit and
        wmf="occluded" take self.despeckled where they took self.occlusion, which stays the LR-check map.  The pipeline
        owns the filter's workspace.  With None nothing is allocated or launched.
        aggregation: None or "sgm" -- None is the reference's guided filter.  "sgm" is semi-global matching (not a stage of
        the reference; include/smx.h smx_dev_sgm_wta_pair; sgm_params: SgmParams, None = the defaults): aggregate() builds
        both WHOLE cost volumes into self.sgm_cost (2, size_d, h, w) -- census with cost="census", else the reference's cost,
        which SGM reads through its clamp to 0 .. 255 -- and runs the one SGM call into self.keys (and self.agg = S,
        self.nbr).  The pipeline owns the volumes and the SGM workspace self.sgm_ws; max_ws_bytes counts both, and a
        slice sub-range or a size that does not fit raises ValueError.  No guided-filter workspace is allocated, self.mean
        stays zero, and radius / eps of `params` are unused.  With None nothing is allocated or launched.
        aggregation="bp" is hierarchical belief propagation (not a stage of the reference; include/smx.h smx_dev_bp_wta_pair;
        bp_params: BpParams, None = the defaults): the flow of "sgm" with the one smx_dev_bp_wta_pair call in its place, the
        whole cost volumes in self.bp_cost and the workspace in self.bp_ws (about 15 bytes per pixel and padded label and view
        at four levels); self.agg receives the belief S.  The same refusals as "sgm".
        uniqueness: None or a ratio > 0 -- the uniqueness (peak-ratio) test (not a stage of the reference; include/smx.h
        smx_dev_uniqueness; OpenCV's uniquenessRatio u is ratio = u / (100 - u)): the aggregation keeps the winners'
        second-best cost in self.uq (2, 3, h, w) through the _uq entries, and finish() runs the test on the LR-checked left map
        into self.unique (vmin = dminl, new_val = dminl - 100) with s - c0 in self.margin.  Order: LR check -> uniqueness ->
        speckle -> fill -> sub-pixel sub_filled -> weighted median: speckle removal takes self.unique where it took
        self.occlusion, which stays the LR-check map, and self.filled is the fill of the last of these maps.  With None nothing
        is allocated or launched.  A slice sub-range (a D-shard) raises ValueError.
        guidance: None or "rgb" -- None is the reference's gray guide.  "rgb" is the colour-guided filter (not a stage of the
        reference; include/smx.h smx_dev_cgf_wta_pair): aggregate() / run() take the colour images rgb_l=, rgb_r= ((h, w, 3 or
        4) uint8 on the device) beside the gray ones, which still give the matching cost, and run cost chunk (the
        reference's cost into self.cgf_cost, or census) -> smx_dev_cgf_wta_pair over chunks of `slices_in_flight` slices.
        The pipeline owns the chunk's cost slices and the workspace self.cgf_ws (max_ws_bytes counts both); no workspace of
        the gray path is allocated and self.mean stays zero.  Not with aggregation="sgm".  With None nothing is allocated or
        launched.
        aggregation="cross" is cross-based aggregation (not a stage of the reference; include/smx.h smx_dev_cross_wta_pair;
        cross_params: CrossParams, None = the defaults): the flow and the buffers of guidance="rgb" -- cost chunk (the
        reference's cost into self.cross_cost, census or AD-Census) -> smx_dev_cross_wta_pair over chunks of
        `slices_in_flight` slices, with the workspace self.cross_ws -- and slice sub-ranges are allowed.  The guide is the
        colour pair rgb_l=, rgb_r= of aggregate() / run() where it is given, else the gray pair.  Not with guidance="rgb".
        vote: None, True (the defaults) or VoteParams -- region voting and 16-direction interpolation on the cross arms (not a
        stage of the reference; include/smx.h smx_dev_region_vote behind the finish; vote_arms: CrossParams whose l1, l2, tau1,
        tau2 build the support regions, None = the defaults): region_vote() behind despeckle() builds the arms of the left guide
        -- the colour image where this aggregate() took one, else the gray one -- into self.vote_arms_plane and votes on the last
        of occlusion / unique / despeckled with self.dmap[1] as the right map, into self.voted; self.filled becomes the fill of
        self.voted.  The validity map is not replaced: the sub-pixel fit and wmf="occluded" take the map they take without
        it.  Works with every aggregation and cost; size_d <= 512.  With None nothing is allocated or launched.
        aggregation="scanline" is the scan-line optimiser with colour-adaptive penalties (not a stage of the reference;
        include/smx.h smx_dev_scanline_wta_pair; scanline_params: ScanlineParams, None = the defaults): the flow of "sgm" --
        both WHOLE cost volumes (the caller's, the reference's cost, census or AD-Census) into self.so_cost (2, size_d, h, w),
        then the one call into self.keys (and self.agg = S, self.nbr, self.uq) with the workspace self.so_ws.  The guide is
        the colour pair rgb_l=, rgb_r= of aggregate() / run() where it is given, else the gray pair.
        aggregation="cross-scanline" is Mei's chain: smx_dev_cross_wta_pair (cross_params) over chunks of `slices_in_flight`
        slices with its q collected into self.so_cost and its keys discarded, then the scan-line optimiser on those volumes,
        which it reads through the clamp: q's four fractional bits are truncated.  max_ws_bytes counts the volumes, the
        workspaces and the chunk buffers; a slice sub-range, more than 256 labels or a size that does not fit raises
        ValueError.
        adjust: None, True (the defaults) or AdjustParams -- the depth-discontinuity adjustment from the aggregated costs (not a
        stage of the reference; include/smx.h smx_dev_discontinuity_adjust): the aggregation keeps its volumes in self.agg as
        with want_agg, whichever aggregation is set, and discontinuity_adjust() runs behind LR check -> uniqueness -> speckle ->
        vote -> fill -> sub-pixel fit and in front of the weighted median, on self.filled with the left volume, into
        self.adjusted; self.filled is rewritten with it, and with subpixel on self.sub_filled carries the changed pixels' own
        fits.  The validity map is not replaced.  max_ws_bytes counts the volumes and the stage's workspace; a slice sub-range
        (a D-shard has no whole volume), more than 512 labels or a size that does not fit raises ValueError.  With None nothing
        is allocated or launched.
        cross_scale: None, True (the defaults: 4 scales, lambda 1.0) or CScaleParams -- cross-scale cost aggregation (Zhang et
        al. 2014; not a stage of the reference; include/smx.h smx_dev_cscale_wta_pair): the guided filter's remedy for
        textureless surfaces wider than its window.  aggregate() keeps the level-0 volumes in self.agg as with want_agg, builds
        the u8 pyramids of both views (smx_dev_pyr_down; the gray pyramid from the gray images, the colour pyramid from the
        colour images), runs levels 1 .. scales-1 through pipelines of their own (self.cs_levels: the same cost, guide and
        params at the level's geometry, both views with the larger of the two views' label counts) and replaces the plain
        winners by the combination pass, which overwrites self.agg with the combined volumes and self.keys, self.nbr and
        self.uq with the winners and states of those.  Everything in finish() runs unchanged behind it.  With the guided filter
        only (gray or rgb guide; the reference, census and AD-Census costs): aggregation= raises ValueError, and so do a slice
        sub-range, caller's cost volumes and a pyramid whose coarsest level is narrower than 2 pixels.  self.mean is level
        0's.  max_ws_bytes bounds each level's pipeline by itself.  With None nothing is allocated or launched.
        aggregation="patchmatch" is PatchMatch stereo (Bleyer et al. 2011; not a stage of the reference; include/smx.h
        smx_dev_patchmatch_pair; pm_params: PMParams, None = the defaults): a disparity plane per pixel in place of cost,
        aggregation and winner-take-all.  aggregate() runs the search into self.pm_planes (2, 3, h, w), self.best (the plane
        costs), self.pm_disp (2, h, w) and self.dmap (the labels); finish() runs the LR check and the fill on the labels,
        speckle removal and region voting behind them unchanged, then self.sub_filled = the left disp where the pixel was
        kept, the filled label elsewhere (smx_dev_pm_sub_filled), then the weighted median.  There is no cost volume: cost=,
        guidance=, cross_scale=, adjust=, uniqueness=, subpixel=, want_agg=, caller's cost volumes and a slice sub-range raise
        ValueError.  self.mean stays zero and self.keys is not written.
        permeability: None, True (the default sigma 32.0, a starting point chosen on a synthetic band) or PermParams -- the
        information permeability filter (Cigla & Alatan 2013; not a stage of the reference; include/smx.h
        smx_dev_permeability_wta_pair): full-image edge-aware aggregation behind the guided filter.  aggregate() keeps the
        aggregated volumes in self.agg as with want_agg, runs the filter in place over them (guide: the gray images, or the
        colour pair with guidance="rgb") and replaces self.keys, self.nbr and self.uq with the winners and states of the
        filtered volumes, whose costs are weighted sums, not means.  Everything in finish() runs unchanged behind it.  With the
        guided filter only (either guide; the reference, census and AD-Census costs): aggregation= and cross_scale= raise
        ValueError, and so does a slice sub-range.  Its workspace (self.perm_ws, at most ~1 GiB: the pass goes in chunks of
        slices) is not counted in max_ws_bytes.  With None nothing is allocated or launched."""
        # (the constructor's own arguments, by name: everything but the device is the plan's)
        args = {k: v for k, v in locals().items() if k not in ("self", "device")}
        self._build(plan_pipeline(_lib.lib(), **args), device)

    @classmethod
    def _from_plan(cls, plan, device):
        self = cls.__new__(cls)
        self._build(plan, device)
        return self

    def _build(self, plan, device):
        """The pipeline of a plan (pipeline_plan.plan_pipeline): its options and byte counts onto the attributes, its buffers
        allocated, the AD-Census table uploaded, and the cross-scale levels built from its sub-plans."""
        self.lib, self.plan, self.device = _lib.lib(), plan, torch.device(device)
        for name, value in {**plan.options, **plan.bytes}.items():
            setattr(self, name, value)
        self._guide = None            # left image of the last aggregation: the guide of the refinement
        self._rgb = None
        new = lambda shape, dtype, zeroed=False: (torch.zeros if zeroed else torch.empty)(shape, dtype=getattr(torch, dtype),
                                                                                         device=self.device)
        for name in BUFFERS:
            setattr(self, name, None)
        for name, shape, dtype, zeroed in plan.buffers:
            setattr(self, name, new(shape, dtype, zeroed))
        if self.adcensus_table is not None:
            with self._on_device():     # a set-up call: it waits for its copy, and stays outside any graph capture
                _lib.check(self.lib.smx_dev_adcensus_tables(C.byref(self.adcensus_params), _dp(self.adcensus_table),
                                                            self._stream()))
        self.cs_levels = [PairPipeline._from_plan(sub, device) for _, sub, _, _ in plan.levels]
        for k in self.cs_levels:        # (the levels take the table of level 0)
            for name in LEVEL_SHARES:
                setattr(k, name, getattr(self, name))
        self.cs_gray = [new(gray, "uint8") for _, _, gray, _ in plan.levels]
        self.cs_rgb = [new(rgb, "uint8") if rgb else None for _, _, _, rgb in plan.levels]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self):
        return torch.cuda.device(self.device)

    # -- stages ------------------------------------------------------------------------------
    def aggregate(self, gray_l, gray_r, cost_l=None, cost_r=None, rgb_l=None, rgb_r=None):
        """The aggregation of this pipeline (_aggregate_level), and with cross_scale on the pyramid's other levels and the
        combination behind it (_cross_scale)."""
        if self.cross_scale and (cost_l is not None or cost_r is not None):
            raise ValueError("cross-scale aggregation builds every level's cost from the pyramid: pass the images only")
        self._aggregate_level(gray_l, gray_r, cost_l, cost_r, rgb_l, rgb_r)
        if self.cross_scale:
            self._cross_scale(gray_l, gray_r)
        if self.permeability:
            self._permeability(gray_l, gray_r)

    def _guides(self, gray_l, gray_r, colour=True):
        """(guide_l, guide_r, channels): the colour pair of this aggregation if it took one (and `colour` lets it guide), else the
        gray pair."""
        if colour and self._rgb is not None:
            return self._rgb[0], self._rgb[1], int(self._rgb[0].shape[2])
        return gray_l, gray_r, 1

    def _permeability(self, gray_l, gray_r):
        """smx_dev_permeability_wta_pair in place over self.agg: the filtered volumes, and self.keys (self.nbr, self.uq) their
        winners (and states).  Guide: the colour pair of this aggregation under guidance="rgb", else the gray images."""
        gl, gr, ch = self._guides(gray_l, gray_r, colour=bool(self.guidance))     # (the colour images of a cost are no guide)
        with self._on_device():
            _lib.check(self.lib.smx_dev_permeability_wta_pair(C.byref(self.permeability), _dp(self.agg[0]), _dp(self.agg[1]),
                                                              _dp(gl), _dp(gr), ch, self.w, self.h, self.dminl, self.dminr,
                                                              self.size_d, _dp(self.keys), _dp(self.agg), _dp(self.nbr),
                                                              _dp(self.uq), _dp(self.perm_ws), self.perm_ws_bytes, self._stream()))

    def _cross_scale(self, gray_l, gray_r):
        """Levels 1 .. of both views' pyramids through self.cs_levels, then smx_dev_cscale_wta_pair over every level's volumes:
        self.agg becomes the combined volumes, self.keys (self.nbr, self.uq) their winners (and states)."""
        L = self.lib
        below, bw, bh = ((gray_l, gray_r), self._rgb), self.w, self.h
        for k, gray, buf in zip(self.cs_levels, self.cs_gray, self.cs_rgb):
            rgb = None
            with self._on_device():
                st = self._stream()
                for v in range(2):
                    _lib.check(L.smx_dev_pyr_down(_dp(below[0][v]), _dp(gray[v]), bw, bh, 1, st))
                if below[1] is not None:
                    ch = int(below[1][0].shape[2])
                    rgb = buf[:2 * k.n * ch].view(2, k.h, k.w, ch)
                    for v in range(2):
                        _lib.check(L.smx_dev_pyr_down(_dp(below[1][v]), _dp(rgb[v]), bw, bh, ch, st))
            if rgb is None:
                k.aggregate(gray[0], gray[1])
            else:
                k.aggregate(gray[0], gray[1], rgb_l=rgb[0], rgb_r=rgb[1])
            below, bw, bh = ((gray[0], gray[1]), None if rgb is None else (rgb[0], rgb[1])), k.w, k.h
        S = self.cross_scale.scales
        views = [(C.c_void_p * S)(*([self.agg[v].data_ptr()] + [k.agg[v].data_ptr() for k in self.cs_levels])) for v in range(2)]
        with self._on_device():
            _lib.check(L.smx_dev_cscale_wta_pair(C.byref(self.cross_scale), views[0], views[1], self.w, self.h, self.dminl,
                                                 self.dminr, self.size_d, _dp(self.keys), _dp(self.agg), _dp(self.nbr),
                                                 _dp(self.uq), self._stream()))

    def _aggregate_level(self, gray_l, gray_r, cost_l=None, cost_r=None, rgb_l=None, rgb_r=None):
        """Cost build (fused unless cost_* given) + guided-filter aggregation + running WTA of this
        rank's slices, both views.  Leaves packed keys in self.keys.  rgb_l / rgb_r: the colour guides of
        guidance="rgb" and the images of the AD term of cost="adcensus" with colour 1 (required then, refused otherwise)."""
        colour_cost = self.cost == "adcensus" and bool(self.adcensus_params.colour)
        self._rgb = None                # (the colour pair of THIS aggregation, where it takes one)
        if self.aggregation == "patchmatch":
            if cost_l is not None or cost_r is not None:
                raise ValueError("PatchMatch stereo reads no cost volume: pass the images only")
            if (rgb_l is None) != (rgb_r is None):
                raise ValueError("pass both colour guides or neither")
            if rgb_l is not None:           # (the guide of region voting; the search itself is gray)
                self._check_rgb(rgb_l, rgb_r)
                self._rgb = (rgb_l, rgb_r)
            return self._patchmatch(gray_l, gray_r)
        if self.guidance:
            if rgb_l is None or rgb_r is None:
                raise ValueError("guidance='rgb' needs the colour images: pass rgb_l= and rgb_r=")
            self._rgb = (rgb_l, rgb_r)
            return self._aggregate_cgf(gray_l, gray_r, rgb_l, rgb_r, cost_l, cost_r)
        if self.aggregation in ("cross", "scanline", "cross-scanline"):
            if (rgb_l is None) != (rgb_r is None):
                raise ValueError("pass both colour guides or neither")
            if colour_cost and rgb_l is None:
                raise ValueError("cost='adcensus' with colour 1 needs the colour images: pass rgb_l= and rgb_r=")
            if rgb_l is not None:
                self._check_rgb(rgb_l, rgb_r)
                self._rgb = (rgb_l, rgb_r)
            if self.aggregation == "scanline":
                return self._aggregate_scanline(gray_l, gray_r, rgb_l, rgb_r, cost_l, cost_r)
            return self._aggregate_cross(gray_l, gray_r, rgb_l, rgb_r, cost_l, cost_r)
        if colour_cost:
            if rgb_l is None or rgb_r is None:
                raise ValueError("cost='adcensus' with colour 1 needs the colour images: pass rgb_l= and rgb_r=")
            self._check_rgb(rgb_l, rgb_r)
            self._rgb = (rgb_l, rgb_r)
        elif rgb_l is not None or rgb_r is not None:
            raise ValueError("rgb_l / rgb_r are the guides of guidance='rgb': this pipeline has the gray guide")
        # (no smx_dev_init_keys launch: the aggregation presets the keys itself, smx_set_keys_fresh)
        if self.cost and (cost_l is not None or cost_r is not None):
            raise ValueError("a census pipeline builds its own cost volumes: pass the images only")
        if self.aggregation in ("sgm", "bp"):
            return self._aggregate_sgm(gray_l, gray_r, cost_l, cost_r)
        self.lib.smx_set_keys_fresh(1)
        try:
            if self.cost:
                self._aggregate_census(gray_l, gray_r)
            elif cost_l is None and cost_r is None:
                self.aggregate_pair(gray_l, gray_r)
            elif cost_l is not None and cost_r is not None:
                self.aggregate_pair_cost(gray_l, gray_r, cost_l, cost_r)
            else:
                self.aggregate_view(0, gray_l, gray_r, cost_l)
                self.aggregate_view(1, gray_r, gray_l, cost_r)
        finally:
            self.lib.smx_set_keys_fresh(0)

    def _aggregate_call(self, entry, *args):
        """entry(params, *args, stream): an aggregation entry on this pipeline's device and its current stream, with
        `slices_in_flight` as the calling thread's bound on the slices per launch for the time of the call."""
        with self._on_device():
            _lib.check(self.lib.smx_set_max_slices_per_launch(self.slices_in_flight))
            try:
                _lib.check(entry(C.byref(self.params), *args, self._stream()))
            finally:
                self.lib.smx_set_max_slices_per_launch(0)

    def _check_rgb(self, rgb_l, rgb_r):
        for t in (rgb_l, rgb_r):
            if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape[:2]) != (self.h, self.w) or t.shape[2] not in (3, 4) \
                    or not t.is_contiguous():
                raise ValueError(f"a colour guide is a contiguous ({self.h}, {self.w}, 3 or 4) uint8 tensor")
        if rgb_l.shape[2] != rgb_r.shape[2]:
            raise ValueError("both colour guides need the same number of channels")

    def _census_codes(self, gray_l, gray_r, st):
        """The codes of both images into self.codes, a launch per image; nothing for a cost without codes (cost="mi")."""
        for v, g in enumerate((gray_l, gray_r) if self.codes is not None else ()):
            _lib.check(self.lib.smx_dev_census(C.byref(self.census_params), _dp(g), _dp(self.codes[v]), self.w, self.h, 1, st))

    def _code_cost(self, gray_l, gray_r, cl, cr, c0, c1, st):
        """Slices [c0, c1) of both views' cost from self.codes into cl, cr: the census cost, or AD-Census with its AD term from
        the gray images or, with colour 1, from the colour images of this aggregate()."""
        L, w, h = self.lib, self.w, self.h
        if self.cost == "mi":
            _lib.check(L.smx_dev_mi_cost_pair(_dp(self.mi_table), _dp(gray_l), _dp(gray_r), _dp(cl), _dp(cr), w, h, self.dminl,
                                              self.dminr, c0, c1, st))
            return
        if self.cost == "census":
            _lib.check(L.smx_dev_census_cost_pair(C.byref(self.census_params), _dp(self.codes), _dp(cl), _dp(cr), w, h,
                                                  self.dminl, self.dminr, c0, c1, st))
            return
        il, ir = self._rgb if self.adcensus_params.colour else (gray_l, gray_r)
        ch = int(il.shape[2]) if self.adcensus_params.colour else 1
        _lib.check(L.smx_dev_adcensus_cost_pair(C.byref(self.adcensus_params), _dp(self.adcensus_table), _dp(self.codes), _dp(il),
                                                _dp(ir), ch, _dp(cl), _dp(cr), w, h, self.dminl, self.dminr, c0, c1, st))

    def _aggregate_census(self, gray_l, gray_r):
        """The census flow, and AD-Census's: the codes of both images once (one launch where the two images lie back to back in
        memory, else one per image), then per chunk of `slices_in_flight` slices the cost (_code_cost) into self.census_cost
        and the aggregation from it.  Only the first chunk takes the keys as fresh; the later ones accumulate."""
        L = self.lib
        with self._on_device():
            st = self._stream()
            if self.codes is None:          # (the mutual-information cost reads the images themselves)
                pass
            elif gray_r.data_ptr() == gray_l.data_ptr() + self.n:
                _lib.check(L.smx_dev_census(C.byref(self.census_params), _dp(gray_l), _dp(self.codes), self.w, self.h, 2, st))
            else:
                for v, g in enumerate((gray_l, gray_r)):
                    _lib.check(L.smx_dev_census(C.byref(self.census_params), _dp(g), _dp(self.codes[v]), self.w, self.h, 1, st))
        sif = self.slices_in_flight
        for c0 in range(self.s_begin, self.s_end, sif):
            c1 = min(self.s_end, c0 + sif)
            cl, cr = self.census_cost[0], self.census_cost[1]
            with self._on_device():
                self._code_cost(gray_l, gray_r, cl, cr, c0, c1, self._stream())
            whole = self.agg is None or self._agg_chunk is None
            self.aggregate_pair_cost(gray_l, gray_r, cl, cr, c0, c1, self.agg if whole else self._agg_chunk)
            if not whole:
                # (the call wrote its two views c1 - c0 slices apart, whatever the buffer holds)
                flat = self._agg_chunk.view(-1)[:2 * (c1 - c0) * self.n].view(2, c1 - c0, self.h, self.w)
                self.agg[:, c0 - self.s_begin:c1 - self.s_begin].copy_(flat)
            L.smx_set_keys_fresh(0)

    def _aggregate_cgf(self, gray_l, gray_r, rgb_l, rgb_r, cost_l=None, cost_r=None):
        """The colour-guided flow: fresh keys, then per chunk of `slices_in_flight` slices the cost slices of both views
        (the caller's volumes, census, or the reference's cost) and smx_dev_cgf_wta_pair from them, which accumulates into
        the keys (and the neighbour / second-best states)."""
        self._check_rgb(rgb_l, rgb_r)
        self._aggregate_chunks(gray_l, gray_r, cost_l, cost_r, self.cgf_cost, self.lib.smx_dev_cgf_wta_pair, C.byref(self.params),
                               rgb_l, rgb_r, int(rgb_l.shape[2]), self.cgf_ws, self.cgf_ws_bytes)

    def _aggregate_cross(self, gray_l, gray_r, rgb_l, rgb_r, cost_l=None, cost_r=None):
        """The cross-based flow: that of the colour guide with smx_dev_cross_wta_pair; the guide is the colour pair where it is
        given, else the gray pair."""
        gl, gr, ch = self._guides(gray_l, gray_r)
        chain = self.aggregation == "cross-scanline"
        self._aggregate_chunks(gray_l, gray_r, cost_l, cost_r, self.cross_cost, self.lib.smx_dev_cross_wta_pair,
                               C.byref(self.cross_params), gl, gr, ch, self.cross_ws, self.cross_ws_bytes,
                               into=(self.so_cost, self._so_chunk) if chain else None)
        if chain:
            # (the keys of the cross pass are overwritten: the optimiser's are OUT only)
            self._scanline(gl, gr, ch, self.so_cost[0], self.so_cost[1])

    def _aggregate_scanline(self, gray_l, gray_r, rgb_l, rgb_r, cost_l=None, cost_r=None):
        """The scan-line flow: both whole cost volumes (the caller's, census / AD-Census, or the reference's cost), as for SGM,
        and the one smx_dev_scanline_wta_pair call; the guide is the colour pair where it is given, else the gray pair."""
        cl, cr = self._whole_costs(gray_l, gray_r, cost_l, cost_r, self.so_cost)
        self._scanline(*self._guides(gray_l, gray_r), cl, cr)

    def _check_costs(self, cost_l, cost_r):
        if (cost_l is None) != (cost_r is None):
            raise ValueError("pass both cost volumes or neither")
        if self.cost and cost_l is not None:
            raise ValueError("a census pipeline builds its own cost volumes: pass the images only")

    def _whole_costs(self, gray_l, gray_r, cost_l, cost_r, own):
        """Both whole cost volumes of an aggregation that reads them in one call: the caller's, or built into `own` (2, size_d,
        h, w) -- the codes and then the cost of this pipeline over 0 .. size_d, or the reference's cost.  -> (left, right)."""
        self._check_costs(cost_l, cost_r)
        self._guide = gray_l
        if cost_l is not None:
            return cost_l, cost_r
        L, w, h = self.lib, self.w, self.h
        with self._on_device():
            st = self._stream()
            if self.cost:
                self._census_codes(gray_l, gray_r, st)
                self._code_cost(gray_l, gray_r, own[0], own[1], 0, self.size_d, st)
            else:
                P = C.byref(self.params)
                _lib.check(L.smx_dev_cost_volume(P, _dp(gray_l), _dp(gray_r), _dp(own[0]), w, w, h, self.dminl, 0, self.size_d, st))
                _lib.check(L.smx_dev_cost_volume(P, _dp(gray_r), _dp(gray_l), _dp(own[1]), w, w, h, self.dminr, 0, self.size_d, st))
        return own[0], own[1]

    def _scanline(self, guide_l, guide_r, ch, cl, cr):
        with self._on_device():
            _lib.check(self.lib.smx_dev_scanline_wta_pair(
                C.byref(self.so_params), _dp(guide_l), _dp(guide_r), ch, _dp(cl), _dp(cr), self.w, self.h, self.size_d, self.dminl,
                self.dminr, _dp(self.keys), _dp(self.agg), _dp(self.nbr), _dp(self.uq), _dp(self.so_ws), self.so_ws_bytes,
                self._stream()))

    def _aggregate_chunks(self, gray_l, gray_r, cost_l, cost_r, own_cost, entry, params, guide_l, guide_r, ch, ws, ws_bytes,
                          into=None):
        """into: None, or (volumes, chunk buffer or None) of the chain: the aggregated slices go there whatever want_agg says,
        and the neighbour / second-best states are not kept (they belong to the stage behind).
        Fresh keys, then per chunk of `slices_in_flight` slices the cost slices of both views (the caller's volumes, census /
        AD-Census into self.census_cost, or the reference's cost into own_cost) and `entry` -- smx_dev_cgf_wta_pair or
        smx_dev_cross_wta_pair -- from them, which accumulates into the keys (and the neighbour / second-best states)."""
        self._check_costs(cost_l, cost_r)
        self._guide = gray_l
        L, w, h = self.lib, self.w, self.h
        self.init_keys()
        if self.cost:
            with self._on_device():
                self._census_codes(gray_l, gray_r, self._stream())
        sif = self.slices_in_flight
        for c0 in range(self.s_begin, self.s_end, sif):
            c1 = min(self.s_end, c0 + sif)
            with self._on_device():
                st = self._stream()
                if cost_l is not None:
                    cl, cr = cost_l[c0 - self.s_begin:], cost_r[c0 - self.s_begin:]
                elif self.cost:
                    cl, cr = self.census_cost[0], self.census_cost[1]
                    self._code_cost(gray_l, gray_r, cl, cr, c0, c1, st)
                else:
                    # (own_cost is None in the start pass of cost="mi" with the reference's cost: the chunk buffer is there)
                    cl, cr = (own_cost if own_cost is not None else self.census_cost)[:2]
                    P = C.byref(self.params)
                    _lib.check(L.smx_dev_cost_volume(P, _dp(gray_l), _dp(gray_r), _dp(cl), w, w, h, self.dminl, c0, c1, st))
                    _lib.check(L.smx_dev_cost_volume(P, _dp(gray_r), _dp(gray_l), _dp(cr), w, w, h, self.dminr, c0, c1, st))
            agg, chunk = (self.agg, self._agg_chunk) if into is None else into
            nbr, uq = (self.nbr, self.uq) if into is None else (None, None)
            whole = agg is None or chunk is None
            with self._on_device():
                _lib.check(L.smx_set_max_slices_per_launch(sif))
                try:
                    _lib.check(entry(params, _dp(guide_l), _dp(guide_r), ch, _dp(cl), _dp(cr), w, h, c0, c1, _dp(self.keys),
                                     _dp(agg if whole else chunk), _dp(nbr), _dp(uq), _dp(ws), ws_bytes,
                                     self._stream()))
                finally:
                    L.smx_set_max_slices_per_launch(0)
            if not whole:
                # (the call wrote its two views c1 - c0 slices apart, whatever the buffer holds)
                flat = chunk.view(-1)[:2 * (c1 - c0) * self.n].view(2, c1 - c0, h, w)
                agg[:, c0 - self.s_begin:c1 - self.s_begin].copy_(flat)

    def _aggregate_sgm(self, gray_l, gray_r, cost_l=None, cost_r=None):
        """The SGM flow: both whole cost volumes (the caller's, census, or the reference's cost) and the one
        smx_dev_sgm_wta_pair call, which writes the keys (and S, the neighbour state) of both views.  aggregation="bp" runs the
        same flow with smx_dev_bp_wta_pair in that call's place."""
        L, w, h = self.lib, self.w, self.h
        cl, cr = self._whole_costs(gray_l, gray_r, cost_l, cost_r, self.bp_cost if self.aggregation == "bp" else self.sgm_cost)
        with self._on_device():
            st = self._stream()
            if self.aggregation == "bp":
                _lib.check(L.smx_dev_bp_wta_pair(C.byref(self.bp_params), _dp(cl), _dp(cr), w, h, self.size_d, _dp(self.keys),
                                                 _dp(self.agg), _dp(self.nbr), _dp(self.uq) if self.uniqueness else None,
                                                 _dp(self.bp_ws), self.bp_ws_bytes, st))
                return
            head = (C.byref(self.sgm_params), _dp(cl), _dp(cr), w, h, self.size_d, _dp(self.keys), _dp(self.agg), _dp(self.nbr))
            if self.uniqueness:
                _lib.check(L.smx_dev_sgm_wta_pair_uq(*head, _dp(self.uq), _dp(self.sgm_ws), self.sgm_ws_bytes, st))
            else:
                _lib.check(L.smx_dev_sgm_wta_pair(*head, _dp(self.sgm_ws), self.sgm_ws_bytes, st))

    def aggregate_pair_cost(self, gray_l, gray_r, cost_l, cost_r, s_begin=None, s_end=None, agg=None):
        """Both views per launch from materialised cost volumes of this rank's slices (smx_dev_aggregate_wta_pair_cost):
        the reference's data flow, read p + write q.  s_begin / s_end: a sub-range of the pipeline's slices whose cost
        slices cost_* hold (default: all of them); agg: where its aggregated slices go (default: self.agg)."""
        self._guide = gray_l
        s_begin = self.s_begin if s_begin is None else s_begin
        s_end = self.s_end if s_end is None else s_end
        agg = self.agg if agg is None else agg
        args = (_dp(gray_l), _dp(gray_r), _dp(cost_l), _dp(cost_r), self.w, self.h, self.dminl, self.dminr, s_begin,
                s_end, _dp(self.keys), _dp(self.mean), _dp(agg), _dp(self.ws), self.ws_bytes)
        if self.uniqueness:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair_uq, *args, _dp(self.nbr), _dp(self.uq))
        elif self.subpixel:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair_nbr, *args, _dp(self.nbr))
        else:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair_cost, *args)

    def cost_volumes(self, gray_l, gray_r):
        """The two raw cost volumes of this rank's slices, resident in HBM (smx_dev_cost_volume; main.cu:80-82)."""
        n = self.s_end - self.s_begin
        cl = torch.empty((n, self.h, self.w), dtype=torch.float32, device=self.device)
        cr = torch.empty_like(cl)
        with self._on_device():
            L, P, st = self.lib, C.byref(self.params), self._stream()
            _lib.check(L.smx_dev_cost_volume(P, _dp(gray_l), _dp(gray_r), _dp(cl), self.w, self.w, self.h, self.dminl,
                                             self.s_begin, self.s_end, st))
            _lib.check(L.smx_dev_cost_volume(P, _dp(gray_r), _dp(gray_l), _dp(cr), self.w, self.w, self.h, self.dminr,
                                             self.s_begin, self.s_end, st))
        return cl, cr

    def _patchmatch(self, gray_l, gray_r):
        """The PatchMatch search of both views (smx_dev_patchmatch_pair): planes, plane costs into self.best, disp, and the
        labels into self.dmap."""
        self._guide = gray_l
        with self._on_device():
            _lib.check(self.lib.smx_dev_patchmatch_pair(C.byref(self.params), C.byref(self.pm_params), _dp(gray_l), _dp(gray_r),
                                                        self.w, self.h, self.size_d, self.dminl, self.dminr, _dp(self.pm_planes),
                                                        _dp(self.best), _dp(self.pm_disp), _dp(self.dmap), _dp(self.pm_ws),
                                                        self.pm_ws_bytes, self._stream()))

    def aggregate_pair(self, gray_l, gray_r):
        """Both views per kernel launch (smx_dev_aggregate_wta_pair)."""
        self._guide = gray_l
        args = (self.w, self.h, self.dminl, self.dminr, self.s_begin, self.s_end, _dp(self.keys), _dp(self.mean),
                _dp(self.agg), _dp(self.ws), self.ws_bytes)
        if self.uniqueness:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair_uq, _dp(gray_l), _dp(gray_r), None, None, *args,
                                 _dp(self.nbr), _dp(self.uq))
        elif self.subpixel:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair_nbr, _dp(gray_l), _dp(gray_r), None, None, *args,
                                 _dp(self.nbr))
        else:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_pair, _dp(gray_l), _dp(gray_r), *args)

    def init_keys(self):
        with self._on_device():
            _lib.check(self.lib.smx_dev_init_keys(_dp(self.keys), 2 * self.n, self._stream()))

    def aggregate_view(self, view, guide, other, cost=None):
        if self.uniqueness:
            raise ValueError("the uniqueness state is kept by the pair entries: pass both cost volumes or neither")
        dmin = self.dminl if view == 0 else self.dminr
        if view == 0:
            self._guide = guide
        agg = self.agg[view] if self.agg is not None else None
        args = (_dp(guide), _dp(other), _dp(cost), self.w, self.h, dmin, self.s_begin, self.s_end, _dp(self.keys[view]),
                _dp(self.mean[view]), _dp(agg), _dp(self.ws), self.ws_bytes)
        if self.subpixel:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta_nbr, *args, _dp(self.nbr[view]))
        else:
            self._aggregate_call(self.lib.smx_dev_aggregate_wta, *args)

    def last_chunk(self):
        """(slices per walker launch, walker launches) of this thread's last fused aggregation: what
        `slices_in_flight` came to (guidedFilter.cu:171-238 is a loop over single slices)."""
        c, n = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.smx_last_agg_chunk(C.byref(c), C.byref(n)))
        return c.value, n.value

    def finish(self):
        """Keys -> best/dmap (reference presets, dispSelect rule), LR check, filling: main.cu:112-155 in one
        call (smx_dev_finish_pair: one launch, a row per workgroup).  Behind PatchMatch stereo best and dmap are there
        already: the LR check and the fill run on the labels (main.cu:141-155), and the fractional filled map closes the
        outlier stages."""
        self._finish_maps()
        self._finish_stages()

    def _finish_maps(self):
        """The part of finish() up to the LR check and the fill."""
        with self._on_device():
            L, P, st = self.lib, C.byref(self.params), self._stream()
            if self.aggregation == "patchmatch":
                self.occlusion.copy_(self.dmap[0])
                _lib.check(L.smx_dev_detect_occlusion(P, _dp(self.occlusion), _dp(self.dmap[1]), self.dminl - 100, self.w, self.h, st))
                self._fill_from(self.occlusion, st)
            else:
                _lib.check(L.smx_dev_finish_pair(P, _dp(self.keys), self.w, self.h, self.dminl, self.dminr,
                                                 self.dminl - 100, float(self.dminl), _dp(self.best), _dp(self.dmap),
                                                 _dp(self.occlusion), _dp(self.filled), st))

    def _fill_from(self, src, st):
        """self.filled = the fill of the map `src` (main.cu:153-155)."""
        self.filled.copy_(src)
        _lib.check(self.lib.smx_dev_fill_occlusion(_dp(self.filled), self.w, self.h, float(self.dminl), st))

    def _finish_stages(self):
        """The opt-in stages of finish() behind the LR check and the fill."""
        if self.aggregation == "patchmatch":
            if self.speckle:
                self.despeckle()
            if self.vote:
                self.region_vote()
            with self._on_device():
                _lib.check(self.lib.smx_dev_pm_sub_filled(_dp(self.pm_disp[0]), _dp(self._kept()), _dp(self.filled), self.w, self.h,
                                                          self.dminl, _dp(self.sub_filled), self._stream()))
            if self.wmf:
                self.refine()
            return
        if self.uniqueness:
            self.uniqueness_filter()
        if self.speckle:
            self.despeckle()
        if self.vote:
            self.region_vote()
        if self.subpixel:
            self.subpixel_maps()
        if self.adjust:
            self.discontinuity_adjust()
        if self.wmf:
            self.refine()

    def uniqueness_filter(self):
        """self.unique = the LR-checked left map without the pixels whose winner fails the uniqueness test
        (smx_dev_uniqueness on the left view's keys and state, one launch), self.margin = s - c0, and -- unless speckle removal
        follows, which does it -- self.filled rewritten as the fill of that map."""
        with self._on_device():
            L, st = self.lib, self._stream()
            _lib.check(L.smx_dev_uniqueness(self.uniqueness, _dp(self.keys[0]), _dp(self.uq[0]), _dp(self.occlusion),
                                            _dp(self.unique), _dp(self.margin), self.w, self.h, float(self.dminl),
                                            float(self.dminl - 100), st))
            if not self.speckle:
                self._fill_from(self.unique, st)

    def despeckle(self):
        """self.despeckled = the LR-checked (and, with uniqueness on, uniqueness-filtered) left map without its small connected
        components (smx_dev_speckle_filter), and self.filled rewritten as the fill of that map."""
        with self._on_device():
            L, st = self.lib, self._stream()
            src = self.unique if self.uniqueness else self.occlusion
            _lib.check(L.smx_dev_speckle_filter(C.byref(self.speckle), _dp(src), _dp(self.despeckled), self.w,
                                                self.h, float(self.dminl), float(self.dminl - 100), _dp(self.speckle_ws),
                                                self.speckle_ws_bytes, st))
            self._fill_from(self.despeckled, st)

    def region_vote(self):
        """self.voted = the last of the LR-checked / uniqueness-filtered / despeckled left maps with its outliers voted on by
        their cross regions and interpolated along 16 directions (smx_dev_cross_arms on the left guide of the last
        aggregate(), then smx_dev_region_vote), and self.filled rewritten as the fill of that map."""
        if self._guide is None:
            raise RuntimeError("region_vote() needs the left image: run an aggregation first")
        guide, _, ch = self._guides(self._guide, None)
        with self._on_device():
            L, st = self.lib, self._stream()
            _lib.check(L.smx_dev_cross_arms(C.byref(self.vote_arms), _dp(guide), None, ch, self.w, self.h, _dp(self.vote_arms_plane),
                                            st))
            _lib.check(L.smx_dev_region_vote(C.byref(self.vote), _dp(self.vote_arms_plane), _dp(guide), ch, _dp(self._kept()),
                                             _dp(self.dmap[1]), _dp(self.voted), self.w, self.h, self.dminl, self.size_d,
                                             int(self.params.d_lr), _dp(self.vote_ws), self.vote_ws_bytes, st))
            self._fill_from(self.voted, st)

    def _kept(self):
        """The map whose validity test tells which pixels the fill replaced."""
        return self.despeckled if self.speckle else self.unique if self.uniqueness else self.occlusion

    def subpixel_maps(self):
        """Sub-pixel maps of both views from the keys, the neighbour state and the finish's maps (smx_dev_subpixel_pair,
        one launch): self.sub = dmap + delta, self.sub_filled = the left one where the LR check kept the pixel, filled
        where it did not."""
        with self._on_device():
            _lib.check(self.lib.smx_dev_subpixel_pair(_lib.SUBPIX_MODES[self.subpixel], _dp(self.keys), _dp(self.nbr),
                                                      _dp(self.dmap), _dp(self._kept()), _dp(self.filled), self.w,
                                                      self.h, self.dminl, _dp(self.sub), _dp(self.sub_filled),
                                                      self._stream()))

    def discontinuity_adjust(self):
        """self.adjusted = self.filled with the pixels beside its depth steps moved to the neighbour's label where the left
        aggregated volume says that costs them less (smx_dev_discontinuity_adjust, one launch a round); self.filled is
        rewritten with it, and with subpixel on the changed pixels of self.sub_filled become their own fits."""
        with self._on_device():
            mode = _lib.SUBPIX_MODES[self.subpixel] if self.subpixel else 0
            _lib.check(self.lib.smx_dev_discontinuity_adjust(C.byref(self.adjust), _dp(self.filled), _dp(self.agg[0]),
                                                             _dp(self.adjusted), self.w, self.h, self.dminl, self.size_d, mode,
                                                             _dp(self.sub_filled), _dp(self.adjust_ws), self.adjust_ws_bytes,
                                                             self._stream()))
            self.filled.copy_(self.adjusted)

    def refine(self):
        """The weighted median of the filled left map, guided by the left image the last aggregate() saw, into
        self.refined (smx_dev_weighted_median; labels dminl .. dminl + size_d - 1)."""
        if self._guide is None:
            raise RuntimeError("refine() needs the left image: run an aggregation first")
        with self._on_device():
            sel = self._kept() if self.wmf == "occluded" else None
            _lib.check(self.lib.smx_dev_weighted_median(C.byref(self.wmf_params), _dp(self._guide), _dp(self.filled),
                                                        _dp(sel), _dp(self.refined), self.w, self.h, self.dminl,
                                                        self.size_d, self._stream()))

    def finish_per_call(self):
        """The same through the per-stage entry points (the reference's call sequence, seven launches); with the uniqueness
        test or speckle removal on, uniqueness_filter() / despeckle() / region_vote() behind them, as in finish().  The sub-pixel fit, the
        depth-discontinuity adjustment behind it and the weighted median are not run."""
        with self._on_device():
            L, P, st = self.lib, C.byref(self.params), self._stream()
            _lib.check(L.smx_dev_init_wta(_dp(self.best), _dp(self.dmap), 2 * self.n, st))
            _lib.check(L.smx_dev_apply_keys(_dp(self.keys[0]), self.n, self.dminl, _dp(self.best[0]),
                                            _dp(self.dmap[0]), st))
            _lib.check(L.smx_dev_apply_keys(_dp(self.keys[1]), self.n, self.dminr, _dp(self.best[1]),
                                            _dp(self.dmap[1]), st))
            self.occlusion.copy_(self.dmap[0])                                   # main.cu:141
            _lib.check(L.smx_dev_detect_occlusion(P, _dp(self.occlusion), _dp(self.dmap[1]),
                                                  self.dminl - 100, self.w, self.h, st))  # main.cu:149
            self.filled.copy_(self.occlusion)                                    # main.cu:153
            _lib.check(L.smx_dev_fill_occlusion(_dp(self.filled), self.w, self.h, float(self.dminl), st))
        if self.uniqueness:
            self.uniqueness_filter()
        if self.speckle:
            self.despeckle()
        if self.vote:
            self.region_vote()

    def run(self, gray_l, gray_r, rgb_l=None, rgb_r=None):
        if self.cost == "mi":
            self._mi_passes(gray_l, gray_r, rgb_l, rgb_r)
        self.aggregate(gray_l, gray_r, rgb_l=rgb_l, rgb_r=rgb_r)
        self.finish()

    def _mi_passes(self, gray_l, gray_r, rgb_l, rgb_r):
        """What a cost="mi" pair runs before its last pass (include/smx.h, smx_ctx_set_mi): the start map into self.occlusion --
        the random one, or the LR-checked left map of a pass with the reference's cost -- then per table the histogram of
        self.occlusion, its table by way of the host (smx_dev_mi_table waits for the stream: a pair is not graph-capturable)
        and, before the last table, a pass that stops behind the LR check and the fill."""
        L, mp = self.lib, self.mi_params
        if mp.init == _lib.MI_INITS["reference"]:
            levels = [self] + self.cs_levels
            for p in levels:
                p.cost = None
            try:
                self.aggregate(gray_l, gray_r, rgb_l=rgb_l, rgb_r=rgb_r)
            finally:
                for p in levels:
                    p.cost = "mi"
            self._finish_maps()
        else:
            with self._on_device():
                _lib.check(L.smx_dev_mi_random_map(_dp(self.occlusion), self.w, self.h, self.dminl, self.size_d, mp.seed, self._stream()))
        for k in range(1, mp.iterations + 1):
            with self._on_device():
                st = self._stream()
                _lib.check(L.smx_dev_mi_histogram(_dp(gray_l), _dp(gray_r), _dp(self.occlusion), float(self.dminl - 100),
                                                  _dp(self.mi_hist), self.w, self.h, st))
                hist = self.mi_hist.cpu().numpy()
                _lib.check(L.smx_dev_mi_table(hist.ctypes.data, _dp(self.mi_table), st))
            if k < mp.iterations:
                self.aggregate(gray_l, gray_r, rgb_l=rgb_l, rgb_r=rgb_r)
                self._finish_maps()

    def check_status(self):
        """Raise if a workgroup of the fused aggregation gave up waiting for a neighbour."""
        torch.cuda.synchronize(self.device)
        for k in self.cs_levels:
            k.check_status()
        if self.plan.no_walker:                          # (the SGM, colour-guided and cross-based kernels wait for nothing)
            return
        with self._on_device():
            _lib.check(self.lib.smx_dev_agg_status(_dp(self.ws)))

    def results(self):
        """Host copies (numpy) named like the oracle's dict."""
        self.check_status()
        c = lambda t: t.detach().cpu().numpy()
        r = {"bestl": c(self.best[0]), "bestr": c(self.best[1]), "dmapl": c(self.dmap[0]),
             "dmapr": c(self.dmap[1]), "meanl": c(self.mean[0]), "meanr": c(self.mean[1]),
             "occlusion": c(self.occlusion), "filled": c(self.filled)}
        if self.agg is not None:
            r["aggl"], r["aggr"] = c(self.agg[0]), c(self.agg[1])
        if self.wmf:
            r["refined"] = c(self.refined)
        if self.uniqueness:
            r["unique"], r["margin"] = c(self.unique), c(self.margin)
        if self.speckle:
            r["despeckled"] = c(self.despeckled)
        if self.vote:
            r["voted"] = c(self.voted)
        if self.adjust:
            r["adjusted"] = c(self.adjusted)
        if self.subpixel:
            r["subpixl"], r["subpixr"], r["subpix_filled"] = c(self.sub[0]), c(self.sub[1]), c(self.sub_filled)
        if self.aggregation == "patchmatch":
            r["pm_planes"] = c(self.pm_planes)
            r["subpixl"], r["subpixr"], r["subpix_filled"] = c(self.pm_disp[0]), c(self.pm_disp[1]), c(self.sub_filled)
        return r


def zncc_cost_volumes(gray_l, gray_r, size_d, dminl, dminr=0, params=None, s_begin=0, s_end=None):
    """The ZNCC window cost of a pair on the device (include/smx.h smx_dev_zncc_moments, smx_dev_zncc_cost_pair): two launches
    on torch's current stream, the moments of both images and slices [s_begin, s_end) of both views' volumes.  gray_l, gray_r:
    (h, w) uint8 tensors on one GPU.  Returns (cost_l, cost_r), float32 (s_end - s_begin, h, w) with labels dminl + z and
    dminr + z: what PairPipeline.aggregate(gray_l, gray_r, cost_l=..., cost_r=...) takes in every flow."""
    if gray_l.dtype != torch.uint8 or gray_l.dim() != 2 or gray_r.shape != gray_l.shape or gray_r.dtype != torch.uint8:
        raise ValueError("zncc_cost_volumes expects two (h, w) uint8 tensors of one shape")
    if not gray_l.is_cuda or gray_r.device != gray_l.device:
        raise ValueError("zncc_cost_volumes expects both images on one GPU")
    s_end = int(size_d) if s_end is None else int(s_end)
    if not 0 <= s_begin <= s_end <= size_d:
        raise ValueError("zncc_cost_volumes needs 0 <= s_begin <= s_end <= size_d")
    p = params if params is not None else _lib.default_zncc_params()
    L = _lib.lib()
    h, w = gray_l.shape
    dev = gray_l.device
    pair = torch.stack((gray_l, gray_r)).contiguous()
    mom = torch.empty((2, h, w), dtype=torch.int64, device=dev)
    cost = torch.empty((2, s_end - s_begin, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.smx_dev_zncc_moments(C.byref(p), _dp(pair), _dp(mom), w, h, 2, st))
        _lib.check(L.smx_dev_zncc_cost_pair(C.byref(p), _dp(mom), _dp(pair[0]), _dp(pair[1]), _dp(cost[0]), _dp(cost[1]), w, h,
                                            int(dminl), int(dminr), int(s_begin), s_end, st))
    return cost[0], cost[1]


def tree_filter_pair(vol_l, vol_r, guide_l, guide_r, sigma=None, dminl=0, dminr=0, want_states=False):
    """Non-local aggregation of a pair's volumes on the minimum spanning trees of their guides, on the device (include/smx.h
    smx_dev_tree_wta_pair; Yang 2012; not a stage of the reference).  vol_l, vol_r: (size_d, h, w) float32 tensors on one GPU --
    aggregated volumes, or raw cost volumes for the paper's own form; guide_l, guide_r: HOST arrays, (h, w) or
    (h, w, 1 | 3 | 4) uint8: the trees are built on the host (stages.tree_build) and uploaded, which costs more than the
    kernels.  sigma: None (the default 25.5), a float or TreeParams.  The inputs are left as they are: the filter runs in place
    over one copy of both.  Returns (out_l, out_r, keys) -- keys (2, h, w) int64, the packed winners of both views -- and with want_states also the
    neighbour state and the second-best state, (2, 3, h, w) float32 each.  Everything runs on torch's current stream."""
    from . import stages
    if vol_l.dtype != torch.float32 or vol_l.dim() != 3 or vol_r.shape != vol_l.shape or vol_r.dtype != torch.float32:
        raise ValueError("tree_filter_pair expects two (size_d, h, w) float32 tensors of one shape")
    if not vol_l.is_cuda or vol_r.device != vol_l.device or not vol_l.is_contiguous() or not vol_r.is_contiguous():
        raise ValueError("tree_filter_pair expects both volumes contiguous on one GPU")
    p = stages._tree_params(sigma, "tree_filter_pair")
    size_d, h, w = vol_l.shape
    L = _lib.lib()
    dev = vol_l.device
    blobs = []
    for g in (guide_l, guide_r):
        g, _ = stages._tree_guide(g, h, w)
        blobs.append(torch.from_numpy(stages.tree_build(g)))
    ws_bytes = L.smx_tree_workspace_bytes(w, h, size_d, 2) // 2
    if ws_bytes == 0:
        raise ValueError("tree_filter_pair needs w*h < 2^31 and size_d <= 2^20")
    per = 2 * w * h * 4
    ws_bytes = min(ws_bytes, max(per, (1 << 30) // per * per))
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        trees = torch.stack(blobs).to(dev)
        out = torch.stack((vol_l, vol_r))
        keys = torch.empty((2, h, w), dtype=torch.int64, device=dev)
        nbr = torch.empty((2, 3, h, w), dtype=torch.float32, device=dev) if want_states else None
        uq = torch.empty((2, 3, h, w), dtype=torch.float32, device=dev) if want_states else None
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(L.smx_dev_tree_wta_pair(C.byref(p), _dp(out[0]), _dp(out[1]), _dp(trees[0]), _dp(trees[1]), w, h, int(dminl),
                                           int(dminr), size_d, _dp(keys), _dp(out), _dp(nbr), _dp(uq), _dp(ws), ws_bytes, st))
    return (out[0], out[1], keys, nbr, uq) if want_states else (out[0], out[1], keys)
