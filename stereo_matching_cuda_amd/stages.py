"""numpy front end of the host-pointer stage API -- same names, argument meaning and in/out
behaviour as the reference's per-stage host functions (host arrays in, host arrays out,
synchronous).  Every function is a thin call into the C-ABI (include/smx.h); all arithmetic
happens in the HIP kernels.

Reference signatures (stereo_matching_cuda/*.cuh):
  rgb_to_grayscale(h_rgb, n, channels, compare)                       rgb_to_grayscale.cuh:7
  compute_cost(i1, i2, cost, w1, w2, h1, h2, dmin, compare)           costVolume.cuh:7
  compute_guided_filter(i, cost, filter_cost, disp_map, mean, w, h, size_d, dmin, compare)
                                                                       guidedFilter.cuh:7
  integral(image, integral, width, height)                            integral.cuh:3
  detect_occlusion(dL, dR, dOcclusion, dmapl, dmapr, w, h)            occlusion.cuh:8
  fill_occlusion(disparity, w, h, vMin)                               occlusion.cuh:14
"""
import ctypes as C

import numpy as np

from . import _lib

WTA_INIT_BITS = 0x7F7F7F7F  # main.cu:112: memset(best_cost, 9999999.0f, ...) sets every byte to 0x7F


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    a = np.ascontiguousarray(a, dtype=dt)
    return a


def _params(p):
    return p if p is not None else _lib.default_params()


def rgb_to_grayscale(h_rgb, params=None):
    """(h, w, ch>=3) u8 -> (h, w) u8.  rgb_to_grayscale.cu:25-73."""
    rgb = _c(h_rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] < 3:
        raise ValueError("rgb_to_grayscale expects an (h, w, channels>=3) uint8 array")
    h, w, ch = rgb.shape
    gray = np.empty((h, w), np.uint8)
    _lib.check(_lib.lib().smx_rgb_to_grayscale(C.byref(_params(params)), _ptr(rgb), h * w, ch, _ptr(gray)))
    return gray


def compute_cost(i1, i2, size_d, dmin, params=None):
    """Cost volume [z][y][x], slice z has label dmin + z.  costVolume.cu:4-84."""
    i1, i2 = _c(i1, np.uint8), _c(i2, np.uint8)
    if i1.ndim != 2 or i2.ndim != 2:
        raise ValueError("compute_cost expects two (h, w) uint8 images")
    h1, w1 = i1.shape
    h2, w2 = i2.shape
    cost = np.empty((size_d, h1, w1), np.float32)
    _lib.check(_lib.lib().smx_compute_cost(C.byref(_params(params)), _ptr(i1), _ptr(i2), _ptr(cost),
                                           w1, w2, h1, h2, size_d, dmin))
    return cost


def integral(image):
    """Integral image with the reference's sequential f32 addition order.  integral.cu:3-51."""
    image = _c(image, np.float32)
    if image.ndim != 2:
        raise ValueError("integral expects an (h, w) float32 image")
    h, w = image.shape
    out = np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_integral(_ptr(image), _ptr(out), w, h))
    return out


def filter(image, params=None):
    """The reference's dead `filter()` (filter.cu:117-207): direct zero-padded box filter.
    Returns (mean u8, var f32) like its two output arguments."""
    image = _c(image, np.uint8)
    if image.ndim != 2:
        raise ValueError("filter expects an (h, w) uint8 image")
    h, w = image.shape
    mean = np.empty((h, w), np.uint8)
    var = np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_filter(C.byref(_params(params)), _ptr(image), w, h, _ptr(mean), _ptr(var)))
    return mean, var


def init_wta(h, w):
    """best/dmap presets of main.cu:112-118."""
    best = np.full((h, w), WTA_INIT_BITS, np.uint32).view(np.float32)
    dmap = np.zeros((h, w), np.float32)
    return best, dmap


def compute_guided_filter(i, cost, filter_cost, disp_map, dmin, want_agg=False, params=None):
    """Guided-filter aggregation + WTA.  filter_cost/disp_map are updated IN PLACE exactly like the
    reference's in/out arguments; returns (mean_u8, agg or None).  guidedFilter.cu:4-295."""
    i, cost = _c(i, np.uint8), _c(cost, np.float32)
    h, w = i.shape
    size_d = cost.shape[0]
    if cost.shape != (size_d, h, w):
        raise ValueError("cost must be (size_d, h, w)")
    for a in (filter_cost, disp_map):
        if a.dtype != np.float32 or a.shape != (h, w) or not a.flags.c_contiguous:
            raise ValueError("filter_cost/disp_map must be C-contiguous float32 (h, w) arrays")
    mean = np.empty((h, w), np.uint8)
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    _lib.check(_lib.lib().smx_compute_guided_filter(
        C.byref(_params(params)), _ptr(i), _ptr(cost), _ptr(filter_cost), _ptr(disp_map), _ptr(mean),
        _ptr(agg), w, h, size_d, dmin))
    return mean, agg


def colour_guided_filter(rgb, cost, filter_cost, disp_map, dmin, want_agg=False, params=None):
    """Colour-guided filter aggregation + WTA (smx_colour_guided_filter; not a stage of the reference): rgb is the
    (h, w, 3 or 4) uint8 guide.  filter_cost/disp_map are updated IN PLACE like compute_guided_filter's; returns agg or None."""
    rgb, cost = _c(rgb, np.uint8), _c(cost, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] not in (3, 4):
        raise ValueError("colour_guided_filter expects an (h, w, 3 or 4) uint8 guide")
    h, w, ch = rgb.shape
    size_d = cost.shape[0]
    if cost.shape != (size_d, h, w):
        raise ValueError("cost must be (size_d, h, w)")
    for a in (filter_cost, disp_map):
        if a.dtype != np.float32 or a.shape != (h, w) or not a.flags.c_contiguous:
            raise ValueError("filter_cost/disp_map must be C-contiguous float32 (h, w) arrays")
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    _lib.check(_lib.lib().smx_colour_guided_filter(
        C.byref(_params(params)), _ptr(rgb), ch, _ptr(cost), _ptr(filter_cost), _ptr(disp_map), _ptr(agg), w, h, size_d, dmin))
    return agg


def cross_aggregate(guide, cost, filter_cost, disp_map, dmin, want_agg=False, params=None):
    """Cross-based aggregation + WTA (smx_cross_aggregate; not a stage of the reference): guide is the (h, w) gray or
    (h, w, 3 or 4) colour uint8 guide, params a CrossParams (None = the defaults).  filter_cost/disp_map are updated IN PLACE
    like compute_guided_filter's; returns agg or None."""
    guide, cost = _c(guide, np.uint8), _c(cost, np.float32)
    if guide.ndim == 2:
        guide = guide[:, :, None]
    if guide.ndim != 3 or guide.shape[2] not in (1, 3, 4):
        raise ValueError("cross_aggregate expects an (h, w) or (h, w, 1, 3 or 4) uint8 guide")
    h, w, ch = guide.shape
    size_d = cost.shape[0]
    if cost.shape != (size_d, h, w):
        raise ValueError("cost must be (size_d, h, w)")
    for a in (filter_cost, disp_map):
        if a.dtype != np.float32 or a.shape != (h, w) or not a.flags.c_contiguous:
            raise ValueError("filter_cost/disp_map must be C-contiguous float32 (h, w) arrays")
    p = params if params is not None else _lib.default_cross_params()
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    _lib.check(_lib.lib().smx_cross_aggregate(
        C.byref(p), _ptr(guide), ch, _ptr(cost), _ptr(filter_cost), _ptr(disp_map), _ptr(agg), w, h, size_d, dmin))
    return agg


def detect_occlusion(disparity_left, disparity_right, d_occlusion, params=None):
    """LR consistency check; returns the updated copy of disparity_left.  occlusion.cu:17-85."""
    dl = _c(disparity_left, np.float32).copy()
    dr = _c(disparity_right, np.float32)
    h, w = dl.shape
    _lib.check(_lib.lib().smx_detect_occlusion(C.byref(_params(params)), _ptr(dl), _ptr(dr),
                                               int(d_occlusion), w, h))
    return dl


def fill_occlusion(disparity, v_min):
    """Scan-line filling; returns the filled copy.  occlusion.cu:111-132."""
    d = _c(disparity, np.float32).copy()
    h, w = d.shape
    _lib.check(_lib.lib().smx_fill_occlusion(_ptr(d), w, h, float(v_min)))
    return d


def weighted_median(guide, disparity, dmin, size_d, select=None, params=None):
    """Weighted-median refinement of a disparity map (include/smx.h smx_weighted_median; not a stage of the reference).
    guide: (h, w) u8 gray of the view the map belongs to; labels [dmin, dmin + size_d); select: None filters every pixel,
    else the pixels with (int)select < dmin (pass the pair's occlusion map for the LR-invalidated ones).  Returns a new
    (h, w) float32 array."""
    g, d = _c(guide, np.uint8), _c(disparity, np.float32)
    if g.ndim != 2 or d.shape != g.shape:
        raise ValueError("weighted_median expects an (h, w) uint8 guide and an (h, w) float32 map")
    s = None if select is None else _c(select, np.float32)
    if s is not None and s.shape != g.shape:
        raise ValueError("select must have the map's shape")
    h, w = g.shape
    out = np.empty((h, w), np.float32)
    p = params if params is not None else _lib.default_wmf_params()
    _lib.check(_lib.lib().smx_weighted_median(C.byref(p), _ptr(g), _ptr(d), _ptr(s), _ptr(out), w, h, int(dmin),
                                              int(size_d)))
    return out


def speckle_filter(disparity, vmin, new_val, params=None):
    """Speckle removal of a disparity map (include/smx.h smx_speckle_filter; not a stage of the reference): connected
    components of 4-neighbours that count (finite, fill_occlusion's test against vmin) and differ by at most
    params.max_diff; the pixels of components of at most params.max_size pixels become new_val, every other pixel is
    copied bit for bit.  Returns a new (h, w) float32 array."""
    d = _c(disparity, np.float32)
    if d.ndim != 2:
        raise ValueError("speckle_filter expects an (h, w) float32 map")
    h, w = d.shape
    out = np.empty((h, w), np.float32)
    p = params if params is not None else _lib.default_speckle_params()
    _lib.check(_lib.lib().smx_speckle_filter(C.byref(p), _ptr(d), _ptr(out), w, h, float(vmin), float(new_val)))
    return out


def region_vote(disparity, guide, dmin, size_d, disparity_right=None, d_lr=None, params=None, arms=None):
    """Region voting and 16-direction interpolation of a disparity map on the cross arms of `guide` (include/smx.h
    smx_region_vote; not a stage of the reference).  guide: the (h, w) gray or (h, w, 1, 3 or 4) uint8 image of the view the
    map belongs to; labels [dmin, dmin + size_d); disparity_right: the right view's winner-take-all map, or None (every
    remaining outlier is then an occlusion); d_lr: None takes smx_params' default; params: VoteParams; arms: CrossParams
    whose l1, l2, tau1, tau2 build the support regions (None: the defaults).  Returns a new (h, w) float32 array."""
    d = _c(disparity, np.float32)
    g = _c(guide, np.uint8)
    if d.ndim != 2:
        raise ValueError("region_vote expects an (h, w) float32 map")
    if g.ndim not in (2, 3) or g.shape[:2] != d.shape or (g.ndim == 3 and g.shape[2] not in (1, 3, 4)):
        raise ValueError("region_vote expects an (h, w) or (h, w, 1, 3 or 4) uint8 guide of the map's shape")
    r = None if disparity_right is None else _c(disparity_right, np.float32)
    if r is not None and r.shape != d.shape:
        raise ValueError("disparity_right must have the map's shape")
    if params is not None and not isinstance(params, _lib.VoteParams):
        raise ValueError(f"params must be None or VoteParams, not {params!r}")
    if arms is not None and not isinstance(arms, _lib.CrossParams):
        raise ValueError(f"arms must be None or CrossParams, not {arms!r}")
    h, w = d.shape
    ch = 1 if g.ndim == 2 else g.shape[2]
    out = np.empty((h, w), np.float32)
    p = params if params is not None else _lib.default_vote_params()
    lr = _lib.default_params().d_lr if d_lr is None else int(d_lr)
    _lib.check(_lib.lib().smx_region_vote(C.byref(p), None if arms is None else C.byref(arms), _ptr(g), ch, _ptr(d), _ptr(r),
                                          _ptr(out), w, h, int(dmin), int(size_d), lr))
    return out


def discontinuity_adjust(disparity, agg, dmin, params=None, subpixel=None, sub=None):
    """Depth-discontinuity adjustment of a label map from its view's aggregated volume (include/smx.h
    smx_discontinuity_adjust; not a stage of the reference).  disparity: (h, w) float32; agg: (size_d, h, w) float32, slice z
    the label dmin + z; params: AdjustParams (None: the defaults).  subpixel: None, "parabola" or "equiangular" with sub, an
    (h, w) float32 sub-pixel map: the pixels whose label changed get their own fit, every other one is kept.  Returns a new
    (h, w) float32 array, or (map, sub) with sub given."""
    d = _c(disparity, np.float32)
    a = _c(agg, np.float32)
    if d.ndim != 2:
        raise ValueError("discontinuity_adjust expects an (h, w) float32 map")
    if a.ndim != 3 or a.shape[1:] != d.shape:
        raise ValueError("discontinuity_adjust expects a (size_d, h, w) float32 volume of the map's shape")
    if params is not None and not isinstance(params, _lib.AdjustParams):
        raise ValueError(f"params must be None or AdjustParams, not {params!r}")
    if subpixel is not None and subpixel not in _lib.SUBPIX_MODES:
        raise ValueError(f"subpixel must be None, 'parabola' or 'equiangular', not {subpixel!r}")
    if (sub is None) != (subpixel is None):
        raise ValueError("sub and subpixel go together")
    s = None if sub is None else np.array(sub, dtype=np.float32, order="C")
    if s is not None and s.shape != d.shape:
        raise ValueError("sub must have the map's shape")
    h, w = d.shape
    out = np.empty((h, w), np.float32)
    p = params if params is not None else _lib.default_adjust_params()
    _lib.check(_lib.lib().smx_discontinuity_adjust(C.byref(p), _ptr(d), _ptr(a), _ptr(out), w, h, int(dmin), int(a.shape[0]),
                                                   _lib.SUBPIX_MODES[subpixel] if subpixel else 0, _ptr(s)))
    return out if s is None else (out, s)


def pyr_down(image):
    """One level of the cross-scale pyramid (include/smx.h smx_pyr_down; not a stage of the reference).  image: (h, w) or
    (h, w, 1 | 3 | 4) uint8 -> ((h+1)//2, (w+1)//2[, channels]) uint8: taps 1 4 6 4 1 on integers, reflect-101 borders."""
    a = _c(image, np.uint8)
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)) or a.size == 0:
        raise ValueError("pyr_down expects an (h, w) or (h, w, 1 | 3 | 4) uint8 image")
    h, w = a.shape[:2]
    out = np.empty(((h + 1) // 2, (w + 1) // 2) + a.shape[2:], np.uint8)
    _lib.check(_lib.lib().smx_pyr_down(_ptr(a), _ptr(out), w, h, 1 if a.ndim == 2 else a.shape[2]))
    return out


def cross_scale_combine(levels, dmin, params=None):
    """The cross-scale combination of one view's per-level aggregated volumes and its winners (include/smx.h
    smx_cscale_combine; not a stage of the reference).  levels: `scales` float32 volumes, levels[s] of shape
    (size_d_s, h_s, w_s) -- the geometry of smx_cscale_level for the level-0 shape and labels dmin ..; params: CScaleParams
    whose scales is len(levels) (None: the default lambda).  Returns (combined (size_d, h, w) float32, best (h, w) float32,
    label map (h, w) float32)."""
    if params is not None and not isinstance(params, _lib.CScaleParams):
        raise ValueError(f"params must be None or CScaleParams, not {params!r}")
    vols = [_c(v, np.float32) for v in levels]
    if not 1 <= len(vols) <= 5 or any(v.ndim != 3 or v.size == 0 for v in vols):
        raise ValueError("cross_scale_combine expects 1 .. 5 float32 volumes (size_d_s, h_s, w_s)")
    p = _lib.default_cscale_params()
    if params is not None:
        p.lambda_ = params.lambda_
        if params.scales != len(vols):
            raise ValueError(f"params.scales is {params.scales}, but {len(vols)} levels are given")
    p.scales = len(vols)
    size_d, h, w = vols[0].shape
    for s, v in enumerate(vols):
        ws, hs, _, ds = _lib.cscale_level(w, h, dmin, size_d, s)
        if v.shape != (ds, hs, ws):
            raise ValueError(f"level {s} must have shape {(ds, hs, ws)}, not {v.shape}")
    ptrs = (C.c_void_p * len(vols))(*[v.ctypes.data for v in vols])
    out = np.empty((size_d, h, w), np.float32)
    best = np.empty((h, w), np.float32)
    disp = np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_cscale_combine(C.byref(p), ptrs, w, h, int(dmin), size_d, _ptr(out), _ptr(best), _ptr(disp)))
    return out, best, disp


def permeability_filter(volume, guide, sigma=None, dmin=0):
    """The information permeability filter of one f32 volume and its winners (include/smx.h smx_permeability_filter; Cigla &
    Alatan 2013; not a stage of the reference).  volume: (size_d, h, w) float32 -- any volume: an aggregated one, or a raw cost
    volume for the paper's own form; guide: (h, w) or (h, w, 1 | 3 | 4) uint8; sigma: None (the default 32.0, a starting point
    chosen on a synthetic band), a float or PermParams.  Returns (filtered (size_d, h, w) float32 -- weighted sums, not means --,
    best (h, w) float32, label map (h, w) float32 = dmin + winning slice)."""
    p = _lib.default_perm_params()
    if isinstance(sigma, _lib.PermParams):
        p.sigma = sigma.sigma
    elif sigma is not None:
        p.sigma = float(sigma)
    if not (0.0 < p.sigma < float("inf")):
        raise ValueError(f"permeability_filter needs a finite sigma > 0, not {p.sigma!r}")
    v = _c(volume, np.float32)
    g = _c(guide, np.uint8)
    if v.ndim != 3 or v.size == 0:
        raise ValueError("permeability_filter expects a (size_d, h, w) float32 volume")
    size_d, h, w = v.shape
    if g.ndim not in (2, 3) or g.shape[:2] != (h, w) or (g.ndim == 3 and g.shape[2] not in (1, 3, 4)):
        raise ValueError(f"the guide must be ({h}, {w}) or ({h}, {w}, 1 | 3 | 4) uint8, not {g.shape}")
    out = np.empty((size_d, h, w), np.float32)
    best = np.empty((h, w), np.float32)
    disp = np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_permeability_filter(C.byref(p), _ptr(v), _ptr(g), 1 if g.ndim == 2 else g.shape[2], w, h, int(dmin),
                                                  size_d, _ptr(out), _ptr(best), _ptr(disp)))
    return out, best, disp


def _tree_params(sigma, who):
    p = _lib.default_tree_params()
    if isinstance(sigma, _lib.TreeParams):
        p.sigma = sigma.sigma
    elif sigma is not None:
        p.sigma = float(sigma)
    if not (0.0 < p.sigma < float("inf")):
        raise ValueError(f"{who} needs a finite sigma > 0, not {p.sigma!r}")
    return p


def _tree_guide(guide, h=None, w=None):
    g = _c(guide, np.uint8)
    if g.ndim not in (2, 3) or g.size == 0 or (g.ndim == 3 and g.shape[2] not in (1, 3, 4)) or (h is not None and g.shape[:2] != (h, w)):
        hw = "h, w" if h is None else f"{h}, {w}"
        raise ValueError(f"the guide must be ({hw}) or ({hw}, 1 | 3 | 4) uint8, not {g.shape}")
    return g, 1 if g.ndim == 2 else g.shape[2]


def tree_build(guide):
    """The minimum spanning tree of a guide as the blob of include/smx.h (smx_tree_build: host only, no device call).  guide:
    (h, w) or (h, w, 1 | 3 | 4) uint8.  Returns a uint8 array of smx_tree_bytes(w, h) bytes, 4-byte aligned, which is copied to
    the device as it is."""
    g, ch = _tree_guide(guide)
    h, w = g.shape[:2]
    nbytes = _lib.lib().smx_tree_bytes(w, h)
    if nbytes == 0:
        raise ValueError("tree_build needs w*h < 2^31")
    blob = np.zeros(nbytes // 4, np.uint32)
    _lib.check(_lib.lib().smx_tree_build(_ptr(g), ch, w, h, _ptr(blob)))
    return blob.view(np.uint8)


def tree_filter(volume, guide, sigma=None, dmin=0):
    """Non-local aggregation of one f32 volume on the guide's minimum spanning tree, and its winners (include/smx.h
    smx_tree_filter; Yang 2012; not a stage of the reference).  volume: (size_d, h, w) float32 -- any volume: an aggregated one, or
    a raw cost volume for the paper's own form; guide: (h, w) or (h, w, 1 | 3 | 4) uint8; sigma: None (the default 25.5, the
    paper's 0.1 of the gray range: a starting point), a float or TreeParams.  Returns (filtered (size_d, h, w) float32 -- weighted
    sums, not means --, best (h, w) float32, label map (h, w) float32 = dmin + winning slice)."""
    p = _tree_params(sigma, "tree_filter")
    v = _c(volume, np.float32)
    if v.ndim != 3 or v.size == 0:
        raise ValueError("tree_filter expects a (size_d, h, w) float32 volume")
    size_d, h, w = v.shape
    g, ch = _tree_guide(guide, h, w)
    out = np.empty((size_d, h, w), np.float32)
    best = np.empty((h, w), np.float32)
    disp = np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_tree_filter(C.byref(p), _ptr(v), _ptr(g), ch, w, h, int(dmin), size_d, _ptr(out), _ptr(best),
                                          _ptr(disp)))
    return out, best, disp


def uniqueness_filter(keys, sec, disparity, ratio, vmin, new_val, want_margin=False):
    """The uniqueness (peak-ratio) test on a disparity map (include/smx.h smx_uniqueness_filter; not a stage of the
    reference).  keys: (h, w) int64 packed WTA keys of the view; sec: (h, w) float32, the winners' second-best cost (plane 0
    of the view's uniqueness state); a pixel whose map value counts against vmin and whose winner has
    sec - c0 < ratio * |c0| becomes new_val, every other pixel is copied bit for bit.  Returns a new (h, w) float32 array,
    or (map, margin) with want_margin."""
    d = _c(disparity, np.float32)
    if d.ndim != 2:
        raise ValueError("uniqueness_filter expects an (h, w) float32 map")
    k, s = _c(keys, np.int64), _c(sec, np.float32)
    if k.shape != d.shape or s.shape != d.shape:
        raise ValueError("keys and sec must have the map's shape")
    h, w = d.shape
    out = np.empty((h, w), np.float32)
    margin = np.empty((h, w), np.float32) if want_margin else None
    _lib.check(_lib.lib().smx_uniqueness_filter(float(ratio), _ptr(k), _ptr(s), _ptr(d), _ptr(out), _ptr(margin), w, h,
                                                float(vmin), float(new_val)))
    return (out, margin) if want_margin else out


def wmf_weights(params=None):
    """(spatial[0 .. 2 r^2], range[0 .. 255]) uint16 weight tables of the weighted median (smx_wmf_weights)."""
    p = params if params is not None else _lib.default_wmf_params()
    spatial = np.zeros(2 * max(p.radius, 0) ** 2 + 1, np.uint16)
    rng = np.zeros(256, np.uint16)
    _lib.check(_lib.lib().smx_wmf_weights(C.byref(p), _ptr(spatial), _ptr(rng)))
    return spatial, rng


def census_transform(img, params=None):
    """Census codes of an (h, w) u8 image -> (h, w) uint64 (include/smx.h smx_dev_census; not a stage of the reference).
    Device buffers come from torch; the transform is the HIP kernel."""
    import torch
    img = _c(img, np.uint8)
    if img.ndim != 2:
        raise ValueError("census_transform expects an (h, w) uint8 image")
    h, w = img.shape
    p = params if params is not None else _lib.default_census_params()
    L = _lib.lib()
    bits = L.smx_census_bits(C.byref(p))
    if bits < 0:                                   # bad parameters: an SmxError before anything touches the device
        _lib.check(bits)
    d_img = torch.from_numpy(img).cuda()
    d_code = torch.empty((h, w), dtype=torch.int64, device=d_img.device)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.smx_dev_census(C.byref(p), C.c_void_p(d_img.data_ptr()), C.c_void_p(d_code.data_ptr()), w, h, 1, st))
    return d_code.cpu().numpy().view(np.uint64)


def census_cost(i1, i2, size_d, dmin, params=None):
    """Census / Hamming cost volume of i1 against i2, [z][y][x], slice z has label dmin + z (smx_census_cost; the census
    counterpart of compute_cost)."""
    i1, i2 = _c(i1, np.uint8), _c(i2, np.uint8)
    if i1.ndim != 2 or i2.shape != i1.shape:
        raise ValueError("census_cost expects two (h, w) uint8 images of one shape")
    h, w = i1.shape
    p = params if params is not None else _lib.default_census_params()
    cost = np.empty((max(size_d, 0), h, w), np.float32)
    _lib.check(_lib.lib().smx_census_cost(C.byref(p), _ptr(i1), _ptr(i2), _ptr(cost), w, h, size_d, dmin))
    return cost


def adcensus_tables(params=None):
    """The AD-Census tables (smx_adcensus_tables; host only): a float32 array of 64 + 766 entries, T[k] the census half,
    T[64 + s] the absolute-difference half."""
    p = params if params is not None else _lib.default_adcensus_params()
    t = np.zeros(_lib.ADCENSUS_TABLE_FLOATS, np.float32)
    _lib.check(_lib.lib().smx_adcensus_tables(C.byref(p), _ptr(t)))
    return t


def adcensus_cost(i1, i2, size_d, dmin, params=None):
    """AD-Census cost volume of i1 against i2, [z][y][x], slice z has label dmin + z (smx_adcensus_cost).  The images are
    (h, w) uint8 with params.colour 0, or (h, w, 3 or 4) uint8 with params.colour 1."""
    i1, i2 = _c(i1, np.uint8), _c(i2, np.uint8)
    if i1.ndim not in (2, 3) or i2.shape != i1.shape:
        raise ValueError("adcensus_cost expects two (h, w) or two (h, w, channels) uint8 images of one shape")
    h, w = i1.shape[:2]
    ch = 1 if i1.ndim == 2 else i1.shape[2]
    p = params if params is not None else _lib.default_adcensus_params()
    cost = np.empty((max(size_d, 0), h, w), np.float32)
    _lib.check(_lib.lib().smx_adcensus_cost(C.byref(p), _ptr(i1), _ptr(i2), ch, _ptr(cost), w, h, size_d, dmin))
    return cost


def mi_histogram(img_l, img_r, disp, occlusion_mark):
    """The joint histogram (256, 256) uint32 of the pixels that the left map `disp` pairs up: H[L[y][x]][R[y][x + d]] counts
    the pixels whose label d is not `occlusion_mark` and whose partner lies inside the image (smx_mi_histogram)."""
    il, ir, m = _c(img_l, np.uint8), _c(img_r, np.uint8), _c(disp, np.float32)
    if il.ndim != 2 or ir.shape != il.shape or m.shape != il.shape:
        raise ValueError("mi_histogram expects two (h, w) uint8 images and an (h, w) float32 map of one shape")
    h, w = il.shape
    hist = np.empty((_lib.MI_LEVELS, _lib.MI_LEVELS), np.uint32)
    _lib.check(_lib.lib().smx_mi_histogram(_ptr(il), _ptr(ir), _ptr(m), float(occlusion_mark), _ptr(hist), w, h))
    return hist


def mi_table(hist):
    """The cost table (256, 256) uint8 of a joint histogram (smx_mi_table; host only, in double): T[i][k] is the cost of a left
    pixel of value i against a right pixel of value k.  Any map gives a histogram, so a caller's own start works too."""
    hist = _c(hist, np.uint32)
    if hist.shape != (_lib.MI_LEVELS, _lib.MI_LEVELS):
        raise ValueError("mi_table expects a (256, 256) uint32 histogram")
    table = np.empty(hist.shape, np.uint8)
    _lib.check(_lib.lib().smx_mi_table(_ptr(hist), _ptr(table)))
    return table


def mi_cost(table, i1, i2, size_d, dmin, right=False):
    """Mutual-information cost volume of i1 against i2, [z][y][x], slice z has label dmin + z (smx_mi_cost).  With right=True
    i1 is the right image and i2 the left one, and the table is read with the roles swapped."""
    table, i1, i2 = _c(table, np.uint8), _c(i1, np.uint8), _c(i2, np.uint8)
    if table.shape != (_lib.MI_LEVELS, _lib.MI_LEVELS):
        raise ValueError("mi_cost expects a (256, 256) uint8 table")
    if i1.ndim != 2 or i2.shape != i1.shape:
        raise ValueError("mi_cost expects two (h, w) uint8 images of one shape")
    h, w = i1.shape
    cost = np.empty((max(size_d, 0), h, w), np.float32)
    _lib.check(_lib.lib().smx_mi_cost(_ptr(table), _ptr(i1), _ptr(i2), int(bool(right)), _ptr(cost), w, h, size_d, dmin))
    return cost


def zncc_cost(i1, i2, size_d, dmin, params=None):
    """ZNCC window cost volume of i1 against i2, [z][y][x], slice z has label dmin + z (smx_zncc_cost; include/smx.h has the
    definition): 127.5 (1 - rho |rho|) rounded, rho the zero-mean normalised cross-correlation of the two windows; 128 where a
    window is flat, 255 where the partner lies outside the image."""
    i1, i2 = _c(i1, np.uint8), _c(i2, np.uint8)
    if i1.ndim != 2 or i2.shape != i1.shape:
        raise ValueError("zncc_cost expects two (h, w) uint8 images of one shape")
    h, w = i1.shape
    p = params if params is not None else _lib.default_zncc_params()
    cost = np.empty((max(size_d, 0), h, w), np.float32)
    _lib.check(_lib.lib().smx_zncc_cost(C.byref(p), _ptr(i1), _ptr(i2), _ptr(cost), w, h, size_d, dmin))
    return cost


def sgm_aggregate(cost, dmin=0, params=None, want_agg=True):
    """Semi-global matching of one (size_d, h, w) float32 cost volume (smx_sgm_aggregate; include/smx.h has the
    definition).  Returns (agg, best, disp_map): S as float32 [z][y][x] (None without want_agg), the winner's S and
    dmin + z*, z* the last slice of minimal S."""
    c = _c(cost, np.float32)
    if c.ndim != 3:
        raise ValueError("sgm_aggregate expects a (size_d, h, w) float32 volume")
    size_d, h, w = c.shape
    p = params if params is not None else _lib.default_sgm_params()
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    best, disp = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_sgm_aggregate(C.byref(p), _ptr(c), None if agg is None else _ptr(agg), _ptr(best), _ptr(disp),
                                            w, h, size_d, int(dmin)))
    return agg, best, disp


def bp_aggregate(cost, dmin=0, params=None, want_agg=True):
    """Hierarchical belief propagation on one (size_d, h, w) float32 cost volume (smx_bp_aggregate; include/smx.h has the
    definition).  Returns (agg, best, disp_map) as sgm_aggregate does, with the belief S in the place of SGM's sum."""
    c = _c(cost, np.float32)
    if c.ndim != 3:
        raise ValueError("bp_aggregate expects a (size_d, h, w) float32 volume")
    size_d, h, w = c.shape
    p = params if params is not None else _lib.default_bp_params()
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    best, disp = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_bp_aggregate(C.byref(p), _ptr(c), None if agg is None else _ptr(agg), _ptr(best), _ptr(disp),
                                           w, h, size_d, int(dmin)))
    return agg, best, disp


def scanline_optimize(guide_own, guide_other, cost, dmin=0, params=None, want_agg=True):
    """Scan-line optimisation with colour-adaptive penalties of one view's (size_d, h, w) float32 cost volume
    (smx_scanline_optimize; include/smx.h has the definition).  guide_own is that view's guide and guide_other the other
    view's, both (h, w) or (h, w, 1 | 3 | 4) uint8; the partner of (x, y) at slice z is (x + dmin + z, y) in guide_other.
    Returns (agg, best, disp_map) as sgm_aggregate does."""
    c = _c(cost, np.float32)
    g, o = _c(guide_own, np.uint8), _c(guide_other, np.uint8)
    if c.ndim != 3:
        raise ValueError("scanline_optimize expects a (size_d, h, w) float32 volume")
    size_d, h, w = c.shape
    if g.ndim not in (2, 3) or g.shape[:2] != (h, w) or o.shape != g.shape:
        raise ValueError("scanline_optimize expects two (h, w) or two (h, w, channels) uint8 guides of the volume's shape")
    ch = 1 if g.ndim == 2 else g.shape[2]
    p = params if params is not None else _lib.default_scanline_params()
    agg = np.empty((size_d, h, w), np.float32) if want_agg else None
    best, disp = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
    _lib.check(_lib.lib().smx_scanline_optimize(C.byref(p), _ptr(g), _ptr(o), ch, _ptr(c), None if agg is None else _ptr(agg),
                                                _ptr(best), _ptr(disp), w, h, size_d, int(dmin)))
    return agg, best, disp


def stereo_pair(gray_l, gray_r, size_d, dminl=None, dminr=0, want_cost=False, want_agg=False,
                params=None):
    """main.cu:65-155 on two gray images, device-resident between the stages."""
    gl, gr = _c(gray_l, np.uint8), _c(gray_r, np.uint8)
    h, w = gl.shape
    if gr.shape != (h, w):
        raise ValueError("both views must have the same shape")
    if dminl is None:
        dminl = -(size_d - 1)
    vol = (size_d, h, w)
    r = {
        "bestl": np.empty((h, w), np.float32), "bestr": np.empty((h, w), np.float32),
        "dmapl": np.empty((h, w), np.float32), "dmapr": np.empty((h, w), np.float32),
        "meanl": np.empty((h, w), np.uint8), "meanr": np.empty((h, w), np.uint8),
        "occlusion": np.empty((h, w), np.float32), "filled": np.empty((h, w), np.float32),
        "costl": np.empty(vol, np.float32) if want_cost else None,
        "costr": np.empty(vol, np.float32) if want_cost else None,
        "aggl": np.empty(vol, np.float32) if want_agg else None,
        "aggr": np.empty(vol, np.float32) if want_agg else None,
    }
    out = _lib.PairOut()
    for f, k in (("best_l", "bestl"), ("best_r", "bestr"), ("dmap_l", "dmapl"), ("dmap_r", "dmapr"),
                 ("mean_l", "meanl"), ("mean_r", "meanr"), ("occlusion", "occlusion"),
                 ("filled", "filled"), ("cost_l", "costl"), ("cost_r", "costr"),
                 ("agg_l", "aggl"), ("agg_r", "aggr")):
        setattr(out, f, None if r[k] is None else r[k].ctypes.data)
    _lib.check(_lib.lib().smx_stereo_pair(C.byref(_params(params)), _ptr(gl), _ptr(gr), w, h, size_d,
                                          dminl, dminr, C.byref(out)))
    return r


def _pm_views(gray_l, gray_r, who):
    gl, gr = _c(gray_l, np.uint8), _c(gray_r, np.uint8)
    if gl.ndim != 2 or gr.shape != gl.shape:
        raise ValueError(f"{who} expects two (h, w) uint8 images of one shape")
    return gl, gr


def patchmatch(gray_l, gray_r, size_d, dminl=None, dminr=0, pm_params=None, params=None):
    """PatchMatch stereo on two gray images (include/smx.h smx_patchmatch; not a stage of the reference): a disparity plane
    per pixel instead of a label.  -> dict: planes (2, 3, h, w) = (a, b, d0) of the left and the right view, cost, disp and
    label (2, h, w), all float32.  pm_params: PMParams or None for the defaults."""
    gl, gr = _pm_views(gray_l, gray_r, "patchmatch")
    h, w = gl.shape
    if dminl is None:
        dminl = -(size_d - 1)
    pm = pm_params if pm_params is not None else _lib.default_pm_params()
    r = {"planes": np.empty((2, 3, h, w), np.float32), "cost": np.empty((2, h, w), np.float32),
         "disp": np.empty((2, h, w), np.float32), "label": np.empty((2, h, w), np.float32)}
    _lib.check(_lib.lib().smx_patchmatch(C.byref(_params(params)), C.byref(pm), _ptr(gl), _ptr(gr), w, h, int(size_d), int(dminl),
                                         int(dminr), _ptr(r["planes"]), _ptr(r["cost"]), _ptr(r["disp"]), _ptr(r["label"])))
    return r


def pm_plane_cost(gray_l, gray_r, planes, size_d, dminl=None, dminr=0, pm_params=None, params=None):
    """The PatchMatch plane cost of given planes of both views, no search (smx_pm_plane_cost).  planes: (2, 3, h, w) float32,
    (a, b, d0) of the left and the right view.  -> (2, h, w) float32."""
    gl, gr = _pm_views(gray_l, gray_r, "pm_plane_cost")
    h, w = gl.shape
    pl = _c(planes, np.float32)
    if pl.shape != (2, 3, h, w):
        raise ValueError("pm_plane_cost expects planes of shape (2, 3, h, w)")
    if dminl is None:
        dminl = -(size_d - 1)
    pm = pm_params if pm_params is not None else _lib.default_pm_params()
    cost = np.empty((2, h, w), np.float32)
    _lib.check(_lib.lib().smx_pm_plane_cost(C.byref(_params(params)), C.byref(pm), _ptr(gl), _ptr(gr), w, h, int(size_d),
                                            int(dminl), int(dminr), _ptr(pl), _ptr(cost)))
    return cost


def write_mat(mat):
    """Host-side float -> u8 normaliser of main.cu:13-35 (PNG writer input).  The reference's
    loop only lowers `min` on elements that did not raise `max` (`else if`, main.cu:22).
    A map with max == min (a constant one) divides by zero there and converts the result to int, which defines nothing:
    it is all zeros here, like normalise_like_reference (host/helpers.cuh) and orc_write_mat_u8."""
    m = np.ascontiguousarray(mat, dtype=np.float32).ravel()
    prev = np.concatenate(([np.float32(-150000000.0)], np.maximum.accumulate(m)[:-1]))
    prev = np.maximum(prev, np.float32(-150000000.0))
    record = m > prev
    mx = max(np.float32(-150000000.0), m.max())
    rest = m[~record]
    mn = np.float32(150000000.0)
    if rest.size:
        mn = min(mn, rest.min())
    if mx == mn:
        return np.zeros(np.shape(mat), np.uint8)
    c = ((m - np.float32(mn)) * np.float32(255.0) / np.float32(mx - mn)).astype(np.float32)
    return c.astype(np.int32).astype(np.uint8).reshape(np.shape(mat))
