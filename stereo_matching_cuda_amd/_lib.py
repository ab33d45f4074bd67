"""ctypes binding of libsmx_hip.so (the C-ABI declared in include/smx.h).

The HIP library is the product: there is no CPU fallback.  If the shared object is missing the
import fails loudly with the build command; if no HIP device is usable every compute call raises
SmxError (SMX_E_HIP).
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
# The product library.  Diagnostic builds of the same C-ABI (tools/v3_stamps.sh: in-kernel stamps) are
# loaded only when BOTH SMX_LIB_PATH and SMX_ALLOW_LIB_OVERRIDE=1 are set, so that one stray variable
# cannot make the tests run against a different binary.
SO_PATH = os.path.join(_PKG, "_build", "libsmx_hip.so")
if os.environ.get("SMX_LIB_PATH"):
    if os.environ.get("SMX_ALLOW_LIB_OVERRIDE") != "1":
        raise ImportError("SMX_LIB_PATH is set but SMX_ALLOW_LIB_OVERRIDE=1 is not: refusing to load a "
                          "non-product build of libsmx_hip.so")
    SO_PATH = os.environ["SMX_LIB_PATH"]
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "smx.h")


class SmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"smx error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """smx_params (SystemIncludes.h:7-24 of the reference as runtime values)."""
    _fields_ = [("r_w", C.c_double), ("g_w", C.c_double), ("b_w", C.c_double),
                ("alpha", C.c_double), ("th_color", C.c_int), ("th_grad", C.c_int),
                ("radius", C.c_int), ("eps", C.c_double), ("d_lr", C.c_int)]


class WmfParams(C.Structure):
    """smx_wmf_params: the weighted-median refinement (not a stage of the reference)."""
    _fields_ = [("radius", C.c_int), ("sigma_s", C.c_double), ("sigma_c", C.c_double)]


class CensusParams(C.Structure):
    """smx_census_params: the census / Hamming matching cost (not a stage of the reference)."""
    _fields_ = [("rx", C.c_int), ("ry", C.c_int), ("th", C.c_int)]


class AdCensusParams(C.Structure):
    """smx_adcensus_params: the AD-Census matching cost, census plus absolute differences (not a stage of the reference)."""
    _fields_ = [("census", CensusParams), ("lambda_census", C.c_double), ("lambda_ad", C.c_double), ("scale", C.c_double),
                ("colour", C.c_int)]


ADCENSUS_TABLE_FLOATS = 64 + 766      # smx.h SMX_ADCENSUS_TABLE_FLOATS


class MiParams(C.Structure):
    """smx_mi_params: the mutual-information matching cost (not a stage of the reference)."""
    _fields_ = [("iterations", C.c_int), ("init", C.c_int), ("seed", C.c_uint32)]


MI_LEVELS = 256                       # smx.h SMX_MI_LEVELS
MI_INITS = {"random": 0, "reference": 1}


class ZnccParams(C.Structure):
    """smx_zncc_params: the ZNCC window matching cost (not a stage of the reference)."""
    _fields_ = [("rx", C.c_int), ("ry", C.c_int)]


class SpeckleParams(C.Structure):
    """smx_speckle_params: the connected-component speckle filter (not a stage of the reference)."""
    _fields_ = [("max_size", C.c_int), ("max_diff", C.c_float)]


class SgmParams(C.Structure):
    """smx_sgm_params: semi-global matching (not a stage of the reference)."""
    _fields_ = [("p1", C.c_int), ("p2", C.c_int), ("paths", C.c_int)]


class BpParams(C.Structure):
    """smx_bp_params: hierarchical belief propagation (not a stage of the reference)."""
    _fields_ = [("step", C.c_int), ("trunc", C.c_int), ("iterations", C.c_int), ("levels", C.c_int), ("data_scale", C.c_float)]


class ScanlineParams(C.Structure):
    """smx_scanline_params: the scan-line optimiser with colour-adaptive penalties (not a stage of the reference)."""
    _fields_ = [("p1", C.c_int), ("p2", C.c_int), ("tau_so", C.c_int), ("paths", C.c_int)]


class CrossParams(C.Structure):
    """smx_cross_params: cross-based aggregation (not a stage of the reference)."""
    _fields_ = [("l1", C.c_int), ("l2", C.c_int), ("tau1", C.c_int), ("tau2", C.c_int), ("iterations", C.c_int)]


class VoteParams(C.Structure):
    """smx_vote_params: region voting and interpolation on the cross arms (not a stage of the reference)."""
    _fields_ = [("tau_s", C.c_int), ("tau_h_pct", C.c_int), ("iterations", C.c_int), ("interpolate", C.c_int)]


class AdjustParams(C.Structure):
    """smx_adjust_params: the depth-discontinuity adjustment from the aggregated costs (not a stage of the reference)."""
    _fields_ = [("tau_e", C.c_int), ("vertical", C.c_int), ("iterations", C.c_int)]


class CScaleParams(C.Structure):
    """smx_cscale_params: cross-scale cost aggregation (not a stage of the reference)."""
    _fields_ = [("scales", C.c_int), ("lambda_", C.c_double)]


class PMParams(C.Structure):
    """smx_pm_params: PatchMatch stereo, a disparity plane per pixel (not a stage of the reference)."""
    _fields_ = [("radius", C.c_int), ("gamma", C.c_double), ("iterations", C.c_int), ("max_slope", C.c_double),
                ("seed", C.c_uint32)]


class PermParams(C.Structure):
    """smx_perm_params: the information permeability filter (not a stage of the reference)."""
    _fields_ = [("sigma", C.c_double)]


class TreeParams(C.Structure):
    """smx_tree_params: non-local aggregation on the guide's minimum spanning tree (not a stage of the reference)."""
    _fields_ = [("sigma", C.c_double)]


class StageMs(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("upload", "guidance", "aggregation", "wta", "finish", "download", "total")] + \
               [("calls", C.c_int), ("dropped", C.c_int)]


class PairOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "best_l", "best_r", "dmap_l", "dmap_r", "mean_l", "mean_r", "occlusion", "filled",
        "cost_l", "cost_r", "agg_l", "agg_r")]


def build(verbose=False):
    """Compile libsmx_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_PKG, "csrc")] + ([] if verbose else ["-s"])
    subprocess.check_call(cmd)
    return SO_PATH


_vp, _i, _i64, _f, _sz, _u64, _u32 = (C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t,
                                      C.c_uint64, C.c_uint32)
_PP = C.POINTER(Params)
_WP = C.POINTER(WmfParams)
_CP = C.POINTER(CensusParams)
_AP = C.POINTER(AdCensusParams)
_IP = C.POINTER(MiParams)
_ZP = C.POINTER(ZnccParams)
_SP = C.POINTER(SpeckleParams)
_GP = C.POINTER(SgmParams)
_BP = C.POINTER(BpParams)
_XP = C.POINTER(CrossParams)
_VP = C.POINTER(VoteParams)
_LP = C.POINTER(ScanlineParams)
_MP = C.POINTER(PMParams)
_JP = C.POINTER(AdjustParams)
_KP = C.POINTER(CScaleParams)
_ip = C.POINTER(C.c_int)
_EP = C.POINTER(PermParams)
_TP = C.POINTER(TreeParams)

# name -> (restype, argtypes).  Mirrors include/smx.h one to one (tests/test_capi.py checks it).
SIGNATURES = {
    "smx_default_params": (None, [_PP]),
    "smx_last_error": (C.c_char_p, []),
    "smx_version": (C.c_char_p, []),
    "smx_device_count": (_i, []),
    "smx_rgb_to_grayscale": (_i, [_PP, _vp, _i64, _i, _vp]),
    "smx_compute_cost": (_i, [_PP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
    "smx_integral": (_i, [_vp, _vp, _i, _i]),
    "smx_compute_guided_filter": (_i, [_PP, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_detect_occlusion": (_i, [_PP, _vp, _vp, _i, _i, _i]),
    "smx_fill_occlusion": (_i, [_vp, _i, _i, _f]),
    "smx_filter": (_i, [_PP, _vp, _i, _i, _vp, _vp]),
    "smx_dev_filter": (_i, [_PP, _vp, _i, _i, _vp, _vp, _vp]),
    "smx_stereo_pair": (_i, [_PP, _vp, _vp, _i, _i, _i, _i, _i, C.POINTER(PairOut)]),
    "smx_create": (_i, [_PP, _i, _i, _i, C.POINTER(_vp)]),
    "smx_ctx_stereo_pair": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(PairOut)]),
    "smx_destroy": (_i, [_vp]),
    "smx_ctx_set_agg_path": (_i, [_vp, _i]),
    "smx_ctx_stereo_pair_async": (_i, [_vp, _vp, _vp, _i, _i]),
    "smx_ctx_wait": (_i, [_vp, C.POINTER(PairOut), C.POINTER(PairOut)]),
    "smx_dev_rgb_to_grayscale": (_i, [_PP, _vp, _i64, _i, _vp, _vp]),
    "smx_dev_cost_volume": (_i, [_PP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "smx_dev_integral": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "smx_agg_workspace_bytes": (_sz, [_i, _i, _i]),
    "smx_agg_workspace_bytes_for": (_sz, [_PP, _i, _i, _i]),
    "smx_dev_aggregate_wta": (_i, [_PP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_dev_aggregate_wta_pair": (_i, [_PP, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_dev_aggregate_wta_pair_cost": (_i, [_PP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_dev_agg_status": (_i, [_vp]),
    "smx_dev_agg_fallback": (_i, [_vp, C.POINTER(_i)]),
    "smx_dev_init_keys": (_i, [_vp, _i64, _vp]),
    "smx_dev_apply_keys": (_i, [_vp, _i64, _i, _vp, _vp, _vp]),
    "smx_dev_init_wta": (_i, [_vp, _vp, _i64, _vp]),
    "smx_dev_detect_occlusion": (_i, [_PP, _vp, _vp, _i, _i, _i, _vp]),
    "smx_dev_fill_occlusion": (_i, [_vp, _i, _i, _f, _vp]),
    "smx_dev_finish_pair": (_i, [_PP, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "smx_pack_key": (_i64, [_f, _u32]),
    "smx_unpack_key": (None, [_i64, C.POINTER(_f), C.POINTER(_u32)]),
    "smx_set_agg_path": (_i, [_i]),
    "smx_last_agg_path": (_i, []),
    "smx_set_max_slices_per_launch": (_i, [_i]),
    "smx_set_keys_fresh": (_i, [_i]),
    "smx_last_agg_chunk": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "smx_agg_geometry": (_i, [_i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "smx_set_timing": (_i, [_i]),
    "smx_last_agg_ms": (_i, [C.POINTER(_f), C.POINTER(_i)]),
    "smx_stage_times": (_i, [C.POINTER(StageMs)]),
    "smx_default_wmf_params": (None, [_WP]),
    "smx_wmf_weights": (_i, [_WP, _vp, _vp]),
    "smx_weighted_median": (_i, [_WP, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_dev_weighted_median": (_i, [_WP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "smx_dev_aggregate_wta_nbr": (_i, [_PP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "smx_dev_aggregate_wta_pair_nbr": (_i, [_PP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp,
                                           _vp]),
    "smx_dev_subpixel_pair": (_i, [_i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "smx_subpixel_delta": (_f, [_i, _f, _f, _f]),
    "smx_ctx_set_subpixel": (_i, [_vp, _i]),
    "smx_ctx_subpixel_maps": (_i, [_vp, _vp, _vp, _vp]),
    "smx_default_census_params": (None, [_CP]),
    "smx_census_bits": (_i, [_CP]),
    "smx_dev_census": (_i, [_CP, _vp, _vp, _i, _i, _i, _vp]),
    "smx_dev_census_cost_pair": (_i, [_CP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "smx_census_cost": (_i, [_CP, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_cost": (_i, [_vp, _i, _CP]),
    "smx_default_adcensus_params": (None, [_AP]),
    "smx_adcensus_tables": (_i, [_AP, _vp]),
    "smx_dev_adcensus_tables": (_i, [_AP, _vp, _vp]),
    "smx_dev_adcensus_cost_pair": (_i, [_AP, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "smx_adcensus_cost": (_i, [_AP, _vp, _vp, _i, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_adcensus": (_i, [_vp, _AP]),
    "smx_default_mi_params": (None, [_IP]),
    "smx_mi_table": (_i, [_vp, _vp]),
    "smx_dev_mi_table": (_i, [_vp, _vp, _vp]),
    "smx_dev_mi_histogram": (_i, [_vp, _vp, _vp, _f, _vp, _i, _i, _vp]),
    "smx_dev_mi_random_map": (_i, [_vp, _i, _i, _i, _i, _u32, _vp]),
    "smx_dev_mi_cost_pair": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "smx_mi_histogram": (_i, [_vp, _vp, _vp, _f, _vp, _i, _i]),
    "smx_mi_cost": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_mi": (_i, [_vp, _IP]),
    "smx_ctx_mi_table": (_i, [_vp, _vp, _vp]),
    "smx_default_zncc_params": (None, [_ZP]),
    "smx_zncc_window": (_i, [_ZP]),
    "smx_zncc_geometry": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "smx_dev_zncc_moments": (_i, [_ZP, _vp, _vp, _i, _i, _i, _vp]),
    "smx_dev_zncc_cost_pair": (_i, [_ZP, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "smx_zncc_cost": (_i, [_ZP, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_zncc": (_i, [_vp, _ZP]),
    "smx_default_speckle_params": (None, [_SP]),
    "smx_speckle_workspace_bytes": (_sz, [_i, _i]),
    "smx_dev_speckle_filter": (_i, [_SP, _vp, _vp, _i, _i, _f, _f, _vp, _sz, _vp]),
    "smx_speckle_filter": (_i, [_SP, _vp, _vp, _i, _i, _f, _f]),
    "smx_speckle_geometry": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "smx_ctx_set_speckle": (_i, [_vp, _SP]),
    "smx_ctx_speckle_map": (_i, [_vp, _vp]),
    "smx_default_sgm_params": (None, [_GP]),
    "smx_sgm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_sgm_wta_pair": (_i, [_GP, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_sgm_aggregate": (_i, [_GP, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_aggregation": (_i, [_vp, _i, _GP]),
    "smx_default_bp_params": (None, [_BP]),
    "smx_bp_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "smx_dev_bp_wta_pair": (_i, [_BP, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_bp_aggregate": (_i, [_BP, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_bp": (_i, [_vp, _BP]),
    "smx_ctx_bp_held": (_i, [_vp, C.POINTER(_sz)]),
    "smx_dev_aggregate_wta_pair_uq": (_i, [_PP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp,
                                          _vp, _vp]),
    "smx_dev_sgm_wta_pair_uq": (_i, [_GP, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_dev_uniqueness": (_i, [_f, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f, _vp]),
    "smx_uniqueness_filter": (_i, [_f, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _f]),
    "smx_ctx_set_uniqueness": (_i, [_vp, _f]),
    "smx_ctx_uniqueness_map": (_i, [_vp, _vp, _vp]),
    "smx_cgf_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_cgf_wta_pair": (_i, [_PP, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_colour_guided_filter": (_i, [_PP, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_guidance": (_i, [_vp, _i]),
    "smx_ctx_stereo_pair_rgb": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(PairOut)]),
    "smx_default_cross_params": (None, [_XP]),
    "smx_cross_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_cross_arms": (_i, [_XP, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "smx_dev_cross_wta_pair": (_i, [_XP, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_cross_aggregate": (_i, [_XP, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_cross": (_i, [_vp, _XP]),
    "smx_default_vote_params": (None, [_VP]),
    "smx_vote_workspace_bytes": (_sz, [_i, _i]),
    "smx_dev_region_vote": (_i, [_VP, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "smx_region_vote": (_i, [_VP, _XP, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "smx_vote_geometry": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "smx_ctx_set_vote": (_i, [_vp, _VP, _XP]),
    "smx_ctx_vote_map": (_i, [_vp, _vp]),
    "smx_default_scanline_params": (None, [_LP]),
    "smx_scanline_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_scanline_wta_pair": (_i, [_LP, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_scanline_optimize": (_i, [_LP, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "smx_ctx_set_scanline": (_i, [_vp, _LP]),
    "smx_default_adjust_params": (None, [_JP]),
    "smx_adjust_workspace_bytes": (_sz, [_i, _i]),
    "smx_dev_discontinuity_adjust": (_i, [_JP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "smx_discontinuity_adjust": (_i, [_JP, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "smx_adjust_geometry": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "smx_ctx_set_adjust": (_i, [_vp, _JP]),
    "smx_default_cscale_params": (None, [_KP]),
    "smx_cscale_weights": (_i, [_KP, _vp]),
    "smx_cscale_level": (_i, [_i, _i, _i, _i, _i, _ip, _ip, _ip, _ip]),
    "smx_dev_pyr_down": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "smx_pyr_down": (_i, [_vp, _vp, _i, _i, _i]),
    "smx_dev_cscale_wta_pair": (_i, [_KP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "smx_cscale_combine": (_i, [_KP, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "smx_pyr_down_geometry": (_i, [_ip, _ip]),
    "smx_ctx_set_cross_scale": (_i, [_vp, _KP]),
    "smx_ctx_cscale_held": (_i, [_vp, _ip, C.POINTER(_sz)]),
    "smx_default_pm_params": (None, [_MP]),
    "smx_pm_weights": (_i, [_MP, _vp]),
    "smx_pm_hash": (_u32, [_u32, _u32, _u32, _u32]),
    "smx_pm_workspace_bytes": (_sz, [_i, _i]),
    "smx_dev_patchmatch_pair": (_i, [_PP, _MP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_dev_pm_plane_cost": (_i, [_PP, _MP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "smx_patchmatch": (_i, [_PP, _MP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "smx_pm_plane_cost": (_i, [_PP, _MP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "smx_pm_geometry": (_i, [_ip, _ip]),
    "smx_dev_pm_sub_filled": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "smx_ctx_set_patchmatch": (_i, [_vp, _MP]),
    "smx_ctx_patchmatch_maps": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "smx_ctx_pm_held": (_i, [_vp, C.POINTER(_sz)]),
    "smx_default_perm_params": (None, [_EP]),
    "smx_perm_table": (_i, [_EP, _vp]),
    "smx_perm_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_permeability_wta_pair": (_i, [_EP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_permeability_filter": (_i, [_EP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "smx_ctx_set_permeability": (_i, [_vp, _EP]),
    "smx_ctx_perm_held": (_i, [_vp, C.POINTER(_sz)]),
    "smx_default_tree_params": (None, [_TP]),
    "smx_tree_bytes": (_sz, [_i, _i]),
    "smx_tree_build": (_i, [_vp, _i, _i, _i, _vp]),
    "smx_tree_tables": (_i, [_TP, _vp, _vp]),
    "smx_tree_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "smx_dev_tree_wta_pair": (_i, [_TP, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "smx_tree_filter": (_i, [_TP, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "smx_ctx_set_tree": (_i, [_vp, _TP]),
    "smx_ctx_tree_held": (_i, [_vp, C.POINTER(_sz)]),
}

# smx.h SMX_AGG_*: the aggregations by name
AGG_MODES = {"guided": 0, "sgm": 1}

# smx.h SMX_GUIDE_*: the guides of the guided filter by name
GUIDE_MODES = {"gray": 0, "rgb": 1}

# smx.h SMX_COST_*: the matching costs by name
COST_MODES = {"reference": 0, "census": 1}

# smx.h SMX_SUBPIX_*: the sub-pixel fits by name
SUBPIX_MODES = {"parabola": 1, "equiangular": 2}

_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, SONAME
    libamdhip64.so.7).  Two HIP runtimes in one process cannot both own the GPU, and device buffers,
    streams and RCCL come from torch, so when torch is installed its runtime is mapped first and
    libsmx_hip.so (NEEDED libamdhip64.so.7) binds to that same copy.  Without torch (e.g. the C++
    host build) the system runtime under /opt/rocm is used.  SMX_HIP_RUNTIME=system skips this."""
    if os.environ.get("SMX_HIP_RUNTIME", "") == "system":
        return None
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return None
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            return C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError:
        pass
    return None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError(
                f"{SO_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C stereo_matching_cuda_amd/csrc` (needs /opt/rocm/bin/hipcc). "
                "There is no CPU fallback.")
        _preload_torch_hip_runtime()
        L = C.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SmxError(rc, lib().smx_last_error().decode("utf-8", "replace"))


def default_params():
    p = Params()
    lib().smx_default_params(C.byref(p))
    return p


def default_wmf_params():
    p = WmfParams()
    lib().smx_default_wmf_params(C.byref(p))
    return p


def default_census_params():
    p = CensusParams()
    lib().smx_default_census_params(C.byref(p))
    return p


def default_mi_params():
    p = MiParams()
    lib().smx_default_mi_params(C.byref(p))
    return p


def default_zncc_params():
    p = ZnccParams()
    lib().smx_default_zncc_params(C.byref(p))
    return p


def default_adcensus_params():
    p = AdCensusParams()
    lib().smx_default_adcensus_params(C.byref(p))
    return p


def default_speckle_params():
    p = SpeckleParams()
    lib().smx_default_speckle_params(C.byref(p))
    return p


def default_sgm_params():
    p = SgmParams()
    lib().smx_default_sgm_params(C.byref(p))
    return p


def default_bp_params():
    p = BpParams()
    lib().smx_default_bp_params(C.byref(p))
    return p


def default_cross_params():
    p = CrossParams()
    lib().smx_default_cross_params(C.byref(p))
    return p


def default_scanline_params():
    p = ScanlineParams()
    lib().smx_default_scanline_params(C.byref(p))
    return p


def default_vote_params():
    p = VoteParams()
    lib().smx_default_vote_params(C.byref(p))
    return p


def default_adjust_params():
    p = AdjustParams()
    lib().smx_default_adjust_params(C.byref(p))
    return p


def default_cscale_params():
    p = CScaleParams()
    lib().smx_default_cscale_params(C.byref(p))
    return p


def default_pm_params():
    p = PMParams()
    lib().smx_default_pm_params(C.byref(p))
    return p


def default_perm_params():
    p = PermParams()
    lib().smx_default_perm_params(C.byref(p))
    return p


def perm_table(params):
    """The 256 permeabilities exp(-k / sigma) of the permeability filter (smx_perm_table) as a list of floats."""
    t = (C.c_float * 256)()
    check(lib().smx_perm_table(C.byref(params), t))
    return list(t)


def default_tree_params():
    p = TreeParams()
    lib().smx_default_tree_params(C.byref(p))
    return p


def tree_tables(params):
    """The two tables of the tree filter (smx_tree_tables): (t, u) with t[k] = exp(-k / sigma) and u[k] = 1 - exp(-2 k / sigma),
    each a list of 256 floats."""
    t, u = (C.c_float * 256)(), (C.c_float * 256)()
    check(lib().smx_tree_tables(C.byref(params), t, u))
    return list(t), list(u)


def pm_weights(params):
    """The 256 adaptive weights exp(-k / gamma) of PatchMatch stereo (smx_pm_weights) as a list of floats."""
    tab = (C.c_float * 256)()
    check(lib().smx_pm_weights(C.byref(params), tab))
    return list(tab)


def pm_hash(seed, view, pixel, draw):
    """The counter-based hash behind PatchMatch stereo's random numbers (smx_pm_hash)."""
    return int(lib().smx_pm_hash(int(seed) & 0xFFFFFFFF, int(view), int(pixel), int(draw)))


def cscale_level(w, h, dmin, size_d, s):
    """(w_s, h_s, dmin_s, size_d_s): the geometry of level s of a cross-scale pyramid (smx_cscale_level)."""
    out = [C.c_int() for _ in range(4)]
    check(lib().smx_cscale_level(int(w), int(h), int(dmin), int(size_d), int(s), *[C.byref(o) for o in out]))
    return tuple(o.value for o in out)


def cscale_weights(params):
    """The levels' weights (smx_cscale_weights) as a list of `scales` floats."""
    wt = (C.c_float * 5)()
    check(lib().smx_cscale_weights(C.byref(params), wt))
    return list(wt)[:params.scales]


def subpixel_delta(mode, c0, lo, hi):
    """The sub-pixel offset of a winner of cost c0 with neighbours lo, hi (smx_subpixel_delta: the formula of the GPU
    kernel, on the host).  mode: "parabola" or "equiangular"."""
    if mode not in SUBPIX_MODES:
        raise ValueError(f"subpixel mode must be 'parabola' or 'equiangular', not {mode!r}")
    return lib().smx_subpixel_delta(SUBPIX_MODES[mode], c0, lo, hi)
