"""numpy reference of region voting and 16-direction interpolation on the cross arms as include/smx.h defines them
(smx_dev_region_vote): integers throughout.  The histograms come from cross_ref.region_sum over the one-hot planes of the
voters (the aggregation's own horizontal-first region, exactly), the interpolation from plain loops.  A plain helper module,
imported by name: tests/test_vote_cpu.py holds it against a scalar brute force; tests/test_gpu_vote.py holds the kernels
against it, bit for bit.
"""
import numpy as np

import cross_ref
import speckle_ref

F32 = np.float32
DEFAULTS = dict(tau_s=20, tau_h_pct=40, iterations=5, interpolate=1)
MAX_D = 512
DIRECTIONS = ((1, 0), (2, 1), (1, 1), (1, 2), (0, 1), (-1, 2), (-1, 1), (-2, 1),
              (-1, 0), (-2, -1), (-1, -1), (-1, -2), (0, -1), (1, -2), (1, -1), (2, -1))          # (dx, dy)


def params_ok(tau_s, tau_h_pct, iterations, interpolate):
    return tau_s >= 0 and 0 <= tau_h_pct <= 99 and 0 <= iterations <= 8 and interpolate in (0, 1)


def shape_ok(w, h, size_d):
    return w >= 1 and h >= 1 and w * h < 2 ** 31 and 1 <= size_d <= MAX_D


def valid(disp, dmin):
    """the speckle filter's rule with vmin = (float)dmin"""
    return speckle_ref.counts(disp, F32(dmin))


def bins(disp, dmin):
    """(int)disp - dmin as int64 (the conversion truncating toward zero and saturating at the ends of int); 0 where not finite"""
    d = np.ascontiguousarray(disp, F32)
    t = np.trunc(np.where(np.isfinite(d), d, 0).astype(np.float64))
    return np.clip(t, -2147483648.0, 2147483647.0).astype(np.int64) - int(dmin)


def voters(disp, dmin, size_d):
    """(voter mask, bins): a valid pixel votes iff its bin lies in 0 .. size_d - 1"""
    b = bins(disp, dmin)
    return valid(disp, dmin) & (b >= 0) & (b < size_d), b


def unpack_arms(packed):
    """(4, h, w) int64 l, r, u, d of an arms plane as smx_dev_cross_arms packs it"""
    a = np.asarray(packed, np.uint32)
    return np.stack((a & 255, (a >> 8) & 255, (a >> 16) & 255, a >> 24)).astype(np.int64)


def histograms(disp, a, dmin, size_d):
    """(labels, H): the bins that have a voter at all, ascending, and H[i][y][x] = voters of bin labels[i] in the region of
    (y, x) -- the planes of the other bins are zero everywhere"""
    v, b = voters(disp, dmin, size_d)
    labels = np.unique(b[v])
    one_hot = (v[None] & (b[None] == labels[:, None, None])).astype(np.int64)
    return labels, cross_ref.region_sum(one_hot, a, 0) if len(labels) else np.zeros((0,) + v.shape, np.int64)


def vote_round(disp, a, dmin, size_d, tau_s, tau_h_pct, stats=None):
    """M_{k+1} from M_k: one Jacobi round.  stats (a dict) collects the counts of the accepted votes and of the two rejections"""
    d = np.ascontiguousarray(disp, F32)
    out = d.copy()
    outlier = ~valid(d, dmin)
    labels, H = histograms(d, a, dmin, size_d)
    if not len(labels):
        if stats is not None:
            stats["reject_s"] = stats.get("reject_s", 0) + int(outlier.sum())
        return out
    S = H.sum(axis=0)
    top = len(labels) - 1 - np.argmax(H[::-1], axis=0)          # the largest bin among those with the largest count
    best = np.take_along_axis(H, top[None], axis=0)[0]
    enough = S > tau_s
    clear = 100 * best > tau_h_pct * S
    take = outlier & enough & clear
    out[take] = (int(dmin) + labels[top[take]]).astype(F32)
    if stats is not None:
        for k, m in (("accepted", take), ("reject_s", outlier & ~enough & clear), ("reject_h", outlier & enough & ~clear),
                     ("reject_both", outlier & ~enough & ~clear)):
            stats[k] = stats.get(k, 0) + int(m.sum())
    return out


def vote(disp, a, dmin, size_d, tau_s=20, tau_h_pct=40, iterations=5, stats=None, rounds=None):
    """M_iterations; rounds (a list) receives M_1 .. M_iterations"""
    m = np.ascontiguousarray(disp, F32).copy()
    for _ in range(iterations):
        m = vote_round(m, a, dmin, size_d, tau_s, tau_h_pct, stats)
        if rounds is not None:
            rounds.append(m)
    return m


def _channels(guide):
    g = np.asarray(guide)
    if g.ndim == 2:
        g = g[:, :, None]
    assert g.dtype == np.uint8 and g.shape[2] in (1, 3, 4)
    return g[:, :, :3].astype(np.int64)


def mismatch(disp_r, y, x, w, dmin, size_d, d_lr):
    """the LR check's own test over every label of the range, in f32"""
    if disp_r is None:
        return False
    d = int(dmin) + np.arange(size_d, dtype=np.int64)
    d = d[(x + d >= 0) & (x + d < w)]
    with np.errstate(invalid="ignore", over="ignore"):
        return bool((np.abs(d.astype(F32) + np.asarray(disp_r, F32)[y, x + d]) <= F32(d_lr)).any())


def _nearest_voters(v):
    """per direction of DIRECTIONS: (qy, qx) of the first voter on the ray that leaves every pixel in that direction, -1 where
    the ray leaves the image first.  Every pixel's ray at once, a step at a time: the walk of the definition, not per pixel."""
    h, w = v.shape
    ys, xs = np.mgrid[0:h, 0:w]
    out = []
    for dx, dy in DIRECTIONS:
        qy, qx = np.full((h, w), -1, np.int64), np.full((h, w), -1, np.int64)
        walking = np.ones((h, w), bool)
        for t in range(1, max(h, w) + 1):
            py, px = ys + t * dy, xs + t * dx
            inside = walking & (py >= 0) & (py < h) & (px >= 0) & (px < w)
            if not inside.any():
                break
            hit = inside.copy()
            hit[inside] = v[py[inside], px[inside]]
            qy[hit], qx[hit] = py[hit], px[hit]
            walking = inside & ~hit
        out.append((qy, qx))
    return out


def interpolate(disp, guide, disp_r, dmin, size_d, d_lr, stats=None):
    """one pass over the map as a snapshot"""
    d = np.ascontiguousarray(disp, F32)
    h, w = d.shape
    I = _channels(guide)
    out = d.copy()
    v, _ = voters(d, dmin, size_d)
    dr = None if disp_r is None else np.ascontiguousarray(disp_r, F32)
    todo = np.nonzero(~valid(d, dmin))
    near = _nearest_voters(v) if todo[0].size else ()
    for y, x in zip(*todo):
        cand = [(int(qy[y, x]), int(qx[y, x])) for qy, qx in near if qy[y, x] >= 0]
        mm = mismatch(dr, y, x, w, dmin, size_d, d_lr)
        if stats is not None:
            k = "no_candidate" if not cand else "mismatch" if mm else "occlusion"
            stats[k] = stats.get(k, 0) + 1
        if not cand:
            continue
        if mm:
            dist = [int(np.abs(I[q] - I[y, x]).max()) for q in cand]
            q = cand[int(np.argmin(dist))]                  # (the first among equals)
        else:
            vals = [d[q] for q in cand]
            q = cand[int(np.argmax(vals))]                  # (equal values of voters: equal integer parts; see region_vote)
        out[y, x] = d[q]
    return out


def region_vote(disp, packed_arms, guide, disp_r, dmin, size_d, d_lr, tau_s=20, tau_h_pct=40, iterations=5, interpolate_=1,
                stats=None):
    """smx_dev_region_vote.  An occlusion takes the largest candidate VALUE, the first in the order among equal values (equal
    floats have equal bits except +-0, and of two candidates +0 and -0 the first is taken)."""
    assert params_ok(tau_s, tau_h_pct, iterations, interpolate_) and shape_ok(disp.shape[1], disp.shape[0], size_d)
    a = unpack_arms(packed_arms)
    m = vote(disp, a, dmin, size_d, tau_s, tau_h_pct, iterations, stats)
    return interpolate(m, guide, disp_r, dmin, size_d, d_lr, stats) if interpolate_ else m


def region_vote_guide(disp, guide, disp_r, dmin, size_d, d_lr, cross=None, **kw):
    """smx_region_vote: the arms from the guide with cross' l1, l2, tau1, tau2"""
    c = dict(cross_ref.DEFAULTS if cross is None else cross)
    c.pop("iterations", None)
    return region_vote(disp, cross_ref.pack_arms(cross_ref.arms(guide, **c)), guide, disp_r, dmin, size_d, d_lr, **kw)


def chain(orc, e, d_lo, D, guide, vote, arms=None, d_lr=0, z=None, best=None, sec=None, nbr=None, uniqueness=None, speckle=None,
          subpixel=None, wmf=None):
    """main_harness.finish_chain with the stage in its place: LR check -> uniqueness -> speckle -> region voting -> fill ->
    sub-pixel fit / weighted median.  vote: a dict of tau_s, tau_h_pct, iterations, interpolate_ (empty: the defaults); arms: a
    dict of l1, l2, tau1, tau2 (None: the defaults).  Adds e["voted"]; e["filled"] is the fill of it, and the validity map of
    the sub-pixel fit and of wmf "occluded" stays the one finish_chain takes."""
    import main_harness
    import subpix_ref
    import wmf_ref
    main_harness.finish_chain(orc, e, d_lo, D, z=z, best=best, sec=sec, nbr=nbr, uniqueness=uniqueness, speckle=speckle)
    kept = e["despeckled"] if speckle else e["unique"] if uniqueness else e["occlusion"]
    e["voted"] = region_vote_guide(kept, guide, e["dmapr"], d_lo, D, d_lr, cross=arms, **vote)
    e["filled"] = e["final"] = orc.fill_occlusion(e["voted"], d_lo)
    if subpixel:
        _, e["sub_filled"] = subpix_ref.maps(subpix_ref.MODES[subpixel], z, best, nbr[0], nbr[1], e["dmapl"], kept, e["filled"], d_lo)
        e["final"] = e["sub_filled"]
    if wmf:
        e["refined"] = wmf_ref.weighted_median(e["grayl"], e["filled"], d_lo, D, kept if wmf == "occluded" else None)
        e["final"] = e["refined"]
    return e


GUIDES = ("textured", "constant", "checkerboard")
MAPS = ("plain", "messy")


def scene(seed, h, w, dmin, size_d, guide="textured", kind="plain", channels=3, holes=0.25):
    """(guide (h, w[, channels]) uint8, disp (h, w) f32, disp_r (h, w) f32) for the tests: blocks of labels with invalidated
    rectangles and single pixels; messy adds NaN, +-inf, -0, fractions, the label behind the range and values beyond int.  The
    right map is random labels of the mirrored range with NaN, so that some outliers are mismatches and some occlusions."""
    rng = np.random.default_rng(seed)
    if guide == "textured":
        blocks = rng.integers(90, 120, ((h + 7) // 8, (w + 7) // 8, channels))
        g = np.kron(blocks, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w, channels))
    elif guide == "constant":
        g = np.full((h, w, channels), 77, np.int64)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        g = np.where(((yy + xx) % 2 == 0)[:, :, None], 60, 180) * np.ones((1, 1, channels), np.int64)
    g = g.astype(np.uint8)
    if channels == 4:
        g[:, :, 3] = rng.integers(0, 256, (h, w))
    d = (dmin + rng.integers(0, size_d, ((h + 5) // 6, (w + 10) // 11))).astype(F32)
    d = np.kron(d, np.ones((6, 11), F32))[:h, :w].copy()
    m = rng.random((h, w))
    d[m < holes / 2] = dmin - 100
    for _ in range(max(1, int(holes * h * w / 40))):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        d[y0:y0 + int(rng.integers(1, 6)), x0:x0 + int(rng.integers(1, 12))] = dmin - 100
    if kind == "messy":
        m = rng.random((h, w))
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, dmin + size_d, 3e9, -3e9, dmin - 0.5)):
            d[(m >= 0.02 * k) & (m < 0.02 * (k + 1))] = v
        d[(m >= 0.16) & (m < 0.20)] += F32(0.25)
    dr = (-(dmin + rng.integers(0, size_d, (h, w)))).astype(F32)
    dr[rng.random((h, w)) < 0.5] = F32(dmin - 1000)
    dr[rng.random((h, w)) < 0.03] = np.nan
    return np.ascontiguousarray(g[:, :, 0] if channels == 1 else g), d.astype(F32), dr


def fill_rows(disp, vmin):
    """the scan-line fill (fill_occlusion) of a finite map: a pixel with (int)v < vmin takes the larger of the nearest values
    >= vmin to its left and to its right on the row, a side without one counting as vmin"""
    d = np.ascontiguousarray(disp, F32)
    assert np.isfinite(d).all()
    out = d.copy()
    h, w = d.shape
    for y in range(h):
        xs = np.nonzero(d[y] >= F32(vmin))[0]
        for x in np.nonzero(np.trunc(d[y]) < F32(vmin))[0]:
            left, right = xs[xs < x], xs[xs > x]
            out[y, x] = max(d[y, left[-1]] if len(left) else F32(vmin), d[y, right[0]] if len(right) else F32(vmin))
    return out
