"""MI355X-native stereo-pair -> disparity-map path (drop-in for hamza1030/stereo_matching_cuda).

Layout
  csrc/     hand-written HIP kernels (gfx950) + the C-ABI of include/smx.h -> _build/libsmx_hip.so
  host/     C++ mirror of the reference's entry point and per-stage headers (main.cpp,
            costVolume.cuh, guidedFilter.cuh, filter.cuh, integral.cuh, winner_take_all.cuh,
            occlusion.cuh, ...) calling the C-ABI
  stages    numpy front end with the reference's stage names (host pointers in/out)
  device    device-resident pipeline on torch-allocated HBM buffers and HIP streams
  pipeline_plan  what that pipeline refuses, owns and sizes: one table of the opt-in stages, host arithmetic only
  sharded   disparity-slice sharding over ranks + packed-key min all-reduce (RCCL / gloo)
  synth     seeded synthetic stereo pairs

Importing the package does not load the HIP library; the first compute call does, and fails
loudly if it has not been built.
"""
from ._lib import (AdCensusParams, AdjustParams, BpParams, CScaleParams, CensusParams, MiParams, PMParams, PermParams, CrossParams, Params, ScanlineParams, SgmParams, SmxError, SpeckleParams, TreeParams, VoteParams, WmfParams, ZnccParams, build, check,  # noqa: F401
                   default_adcensus_params, default_adjust_params, default_bp_params, default_census_params, default_cscale_params, default_cross_params, default_mi_params, default_params, default_perm_params, default_pm_params, default_scanline_params, default_sgm_params, default_speckle_params, default_tree_params, default_vote_params, default_wmf_params, default_zncc_params, lib,
                   perm_table, pm_hash, pm_weights, subpixel_delta, tree_tables)
from .stages import (adcensus_cost, adcensus_tables, bp_aggregate, census_cost, census_transform, colour_guided_filter, compute_cost, cross_aggregate, compute_guided_filter, cross_scale_combine, detect_occlusion, discontinuity_adjust,  # noqa: F401
                     fill_occlusion, filter, init_wta, integral, mi_cost, mi_histogram, mi_table, patchmatch, permeability_filter, pm_plane_cost, pyr_down, region_vote, rgb_to_grayscale, scanline_optimize, sgm_aggregate, speckle_filter, stereo_pair,
                     tree_build, tree_filter, uniqueness_filter, weighted_median, wmf_weights, write_mat, zncc_cost)

__all__ = ["Params", "SmxError", "build", "default_params", "lib", "rgb_to_grayscale",
           "compute_cost", "compute_guided_filter", "integral", "detect_occlusion", "fill_occlusion",
           "init_wta", "stereo_pair", "write_mat", "filter", "check", "WmfParams", "default_wmf_params",
           "weighted_median", "wmf_weights", "subpixel_delta", "CensusParams", "default_census_params",
           "census_transform", "census_cost", "SpeckleParams", "default_speckle_params", "speckle_filter",
           "SgmParams", "default_sgm_params", "sgm_aggregate", "uniqueness_filter", "colour_guided_filter",
           "AdCensusParams", "default_adcensus_params", "adcensus_tables", "adcensus_cost",
           "CrossParams", "default_cross_params", "cross_aggregate", "VoteParams", "default_vote_params", "region_vote",
           "ScanlineParams", "default_scanline_params", "scanline_optimize",
           "AdjustParams", "default_adjust_params", "discontinuity_adjust",
           "CScaleParams", "default_cscale_params", "pyr_down", "cross_scale_combine",
           "PMParams", "default_pm_params", "pm_weights", "pm_hash", "patchmatch", "pm_plane_cost",
           "PermParams", "default_perm_params", "perm_table", "permeability_filter",
           "TreeParams", "default_tree_params", "tree_tables", "tree_build", "tree_filter",
           "BpParams", "default_bp_params", "bp_aggregate",
           "MiParams", "default_mi_params", "mi_histogram", "mi_table", "mi_cost",
           "ZnccParams", "default_zncc_params", "zncc_cost"]
