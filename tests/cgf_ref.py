"""numpy reference of the colour-guided filter aggregation as include/smx.h defines it (smx_dev_cgf_wta_pair), float32
throughout except the 3 x 3 inverse, which is float64 with every product and sum rounded on its own.  A helper module imported
by name: tests/test_cgf_cpu.py holds it against a float64 direct-sum filter; tests/test_gpu_cgf.py holds the kernels against
it, bit for bit.

  integral   f32, row prefix left to right, then column prefix top to bottom; each a sequential chain acc = v + acc from -0.0f
  box_mean   clamped window, ((S11 - S10) - S01) + S00 with the taps outside the image left out, divided by (float)area
  guidance   once per view: mu[3] (r, g, b) and inv[6] = (A, B, C, D, E, F), the rows (A B C; B D E; C E F) of (Sigma + eps I)^-1
  aggregate  q[z] per slice
  outputs    what one view of the device call writes: agg, keys, nbr, uq
  isoluminant_pair, isoluminant_scene    the scene the feature exists for
  colour_pair    a seeded colour stereo pair
"""
import numpy as np

import subpix_ref
import uniq_ref
from stereo_matching_cuda_amd import synth

F32 = np.float32


def integral(img):
    img = np.asarray(img, F32)
    rows = np.cumsum(img, axis=1, dtype=F32)           # (accumulate is a sequential f32 chain; v + -0.0f == v)
    return np.cumsum(rows, axis=0, dtype=F32)


def _taps(w, h, radius):
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    ymin, ymax = np.maximum(-1, y - radius - 1), np.minimum(h - 1, y + radius)
    xmin, xmax = np.maximum(-1, x - radius - 1), np.minimum(w - 1, x + radius)
    area = ((xmax - xmin) * (ymax - ymin)).astype(F32)
    return ymin, ymax, xmin, xmax, area


def box_mean(S, radius):
    """box_taps / box_eval of smx_kernels.hip on an integral image S"""
    S = np.asarray(S, F32)
    h, w = S.shape
    ymin, ymax, xmin, xmax, area = _taps(w, h, radius)
    hx, hy = xmin >= 0, ymin >= 0
    xm, ym = np.maximum(xmin, 0), np.maximum(ymin, 0)
    val = S[ymax, xmax]
    val = np.where(hx, val - S[ymax, xm], val).astype(F32)
    val = np.where(hy, val - S[ym, xmax], val).astype(F32)
    val = np.where(hx & hy, val + S[ym, xm], val).astype(F32)
    return (val / area).astype(F32)


def _mean(img, radius):
    return box_mean(integral(img), radius)


def planes(rgb):
    """u8 [h][w][channels >= 3] -> the three f32 guide planes I_r, I_g, I_b"""
    rgb = np.asarray(rgb, np.uint8)
    assert rgb.ndim == 3 and rgb.shape[2] in (3, 4), rgb.shape
    return [rgb[:, :, c].astype(F32) for c in range(3)]


def guidance(rgb, radius=9, eps=6.5025):
    """-> (I [3], mu [3], inv [6]) of one view"""
    I = planes(rgb)
    mu = [_mean(c, radius) for c in I]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    v = []
    for i, j in pairs:
        m = _mean((I[i] * I[j]).astype(F32), radius)               # (products of two bytes: exact in f32)
        v.append((m - (mu[i] * mu[j]).astype(F32)).astype(F32))
    f64 = np.float64
    eps = f64(eps)
    a, b, c = v[0].astype(f64) + eps, v[1].astype(f64), v[2].astype(f64)
    d, e, f = v[3].astype(f64) + eps, v[4].astype(f64), v[5].astype(f64) + eps
    with np.errstate(all="ignore"):
        A, B, C = d * f - e * e, c * e - b * f, b * e - c * d
        D, E, F = a * f - c * c, b * c - a * e, a * d - b * b
        det = (a * A + b * B) + c * C
        inv = [(X / det).astype(F32) for X in (A, B, C, D, E, F)]
    return I, mu, inv


def filter_slice(p, I, mu, inv, radius):
    """q of one cost slice p (h, w)"""
    p = np.asarray(p, F32)
    A, B, C, D, E, F = inv
    with np.errstate(all="ignore"):
        mp = _mean(p, radius)
        cov = [(_mean((I[c] * p).astype(F32), radius) - (mu[c] * mp).astype(F32)).astype(F32) for c in range(3)]
        dot = lambda x, y, z: (((x * cov[0]).astype(F32) + (y * cov[1]).astype(F32)).astype(F32) + (z * cov[2]).astype(F32)).astype(F32)
        a = [dot(A, B, C), dot(B, D, E), dot(C, E, F)]
        am = (((a[0] * mu[0]).astype(F32) + (a[1] * mu[1]).astype(F32)).astype(F32) + (a[2] * mu[2]).astype(F32)).astype(F32)
        b = (mp - am).astype(F32)
        ab = [_mean(x, radius) for x in a]
        bb = _mean(b, radius)
        q = (((ab[0] * I[0]).astype(F32) + (ab[1] * I[1]).astype(F32)).astype(F32) + (ab[2] * I[2]).astype(F32)).astype(F32)
        return (q + bb).astype(F32), a, b


def aggregate(rgb, cost, radius=9, eps=6.5025):
    """q [z][y][x] f32 of a cost volume [z][y][x]"""
    cost = np.asarray(cost, F32)
    I, mu, inv = guidance(rgb, radius, eps)
    return np.stack([filter_slice(cost[z], I, mu, inv, radius)[0] for z in range(cost.shape[0])])


def states(q, s_begin=0, s_end=None):
    """From an aggregated volume q (slice z of the volume at q[z]) over [s_begin, s_end): keys (h, w) int64, nbr (3, h, w),
    uq (3, h, w), z (h, w; -1: no winner), best (h, w)."""
    z, c0, lo, hi, last = subpix_ref.winners(q, s_begin, s_end)
    z2, c02, sec, rest, last2, _ = uniq_ref.second_best(q, s_begin, s_end)
    assert np.array_equal(z, z2)
    return {"keys": uniq_ref.pack_keys(c0, z), "nbr": np.stack((lo, hi, last)).astype(F32),
            "uq": np.stack((sec, rest, last2)).astype(F32), "z": z, "best": c0}


def outputs(rgb, cost, radius=9, eps=6.5025):
    """What one view of a fresh smx_dev_cgf_wta_pair call over the whole volume writes."""
    q = aggregate(rgb, cost, radius, eps)
    out = states(q)
    out["agg"] = q
    return out


def isoluminant_pair(gray):
    """Two colours of equal gray value that differ by at least 100 in two channels, by search over r, g at b = 128."""
    r, g = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    cols = np.stack((r, g, np.full_like(r, 128)), axis=-1).astype(np.uint8)
    lum = gray(cols)
    for v in range(256):
        idx = np.argwhere(lum == v)
        if idx.size == 0:
            continue
        lo, hi = idx[np.argmin(idx[:, 0])], idx[np.argmax(idx[:, 0])]
        if abs(int(hi[0]) - int(lo[0])) >= 100 and abs(int(hi[1]) - int(lo[1])) >= 100:
            return cols[tuple(lo)], cols[tuple(hi)], v
    raise AssertionError("no isoluminant pair found")


def isoluminant_scene(gray, w=64, h=32, split=32):
    ca, cb, v = isoluminant_pair(gray)
    rgb = np.empty((h, w, 3), np.uint8)
    rgb[:, :split] = ca
    rgb[:, split:] = cb
    p = np.zeros((1, h, w), np.float32)
    p[:, :, split:] = 1
    return rgb, p, v


def colour_pair(w, h, size_d, seed):
    """A seeded colour stereo pair (h, w, 3) uint8: blurred colour noise, the right image the left one shifted by the
    per-row disparity of synth.row_disparity."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, size=(h, w + size_d, 3), dtype=np.uint8)
    base = np.clip(np.rint(synth._blur(base, 1.5)), 0, 255).astype(np.uint8)
    cols = np.arange(w)[None, :] + synth.row_disparity(h, size_d)[:, None]
    right = np.take_along_axis(base, cols[:, :, None].repeat(3, 2), axis=1)
    return np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(right)
