"""numpy reference of the sub-pixel refinement (smx_dev_aggregate_wta*_nbr + smx_dev_subpixel_pair), float32 throughout.

From an aggregated volume q[D][h][w] and the slice range [s_begin, s_end) that was aggregated (one fresh call, or several
calls over ascending contiguous ranges): the winner (the key's rules: smallest cost, the LAST slice among equal costs,
NaN never wins), its neighbours lo = q[z - 1] and hi = q[z + 1] (NaN outside the range, and for a pixel without a
winner), the offset delta and the maps.  `brute_state` replays the kernels' per-slice state machine pixel by pixel.
"""
import numpy as np

PARABOLA, EQUIANGULAR = 1, 2
MODES = {"parabola": PARABOLA, "equiangular": EQUIANGULAR}
F32 = np.float32
NAN = F32(np.nan)


def winners(q, s_begin=0, s_end=None):
    """-> (z, c0, lo, hi, last): z the absolute winning slice (-1: none), c0 its cost (-0 folded to +0, as in the key),
    lo / hi its neighbours in the range, last = q[s_end - 1]."""
    q = np.asarray(q, F32)
    s_end = q.shape[0] if s_end is None else s_end
    v = q[s_begin:s_end]
    nan = np.isnan(v)
    has = ~nan.all(axis=0)
    m = np.where(nan, F32(np.inf), v).min(axis=0)
    hit = (v == m[None]) & ~nan
    k = v.shape[0] - 1 - np.argmax(hit[::-1], axis=0)             # the last slice of the minimum
    z = np.where(has, s_begin + k, -1)
    kk = np.where(has, k, 0)
    c0 = np.take_along_axis(v, kk[None], 0)[0]
    c0 = np.where(c0 == 0, F32(0), c0).astype(F32)
    lo = np.take_along_axis(v, np.maximum(kk - 1, 0)[None], 0)[0]
    hi = np.take_along_axis(v, np.minimum(kk + 1, v.shape[0] - 1)[None], 0)[0]
    lo = np.where(has & (kk >= 1), lo, NAN).astype(F32)
    hi = np.where(has & (kk + 1 < v.shape[0]), hi, NAN).astype(F32)
    return z, c0, lo, hi, v[-1].copy()


def delta(mode, c0, lo, hi):
    """smx_subpixel_delta, vectorised (float32, same operation order)."""
    c0, lo, hi = (np.asarray(x, F32) for x in (c0, lo, hi))
    with np.errstate(all="ignore"):
        a = lo - c0
        b = hi - c0
        den = (a + b) if mode == PARABOLA else np.fmax(a, b)
        d = (a - b) / (F32(2.0) * den)
    d = np.where(np.isnan(lo) | np.isnan(hi) | ~np.isfinite(d), F32(0), d)
    return d.astype(F32)


def dmap_of(z, c0, dmin):
    """The finish's label map: dmin + z where the key has a winner that passes the reference's preset (main.cu:112)."""
    ok = (z >= 0) & (np.uint32(0x7F7F7F7F).view(F32) >= np.asarray(c0, F32))
    return np.where(ok, (dmin + z).astype(F32), F32(0)).astype(F32)


def kept(occlusion, dminl):
    """True where the LR check kept the pixel: fill_occlusion's test (int)occlusion < dminl does not fire (NaN, +-inf: kept)."""
    o = np.asarray(occlusion, F32)
    with np.errstate(invalid="ignore"):
        dropped = np.isfinite(o) & (np.trunc(o.astype(np.float64)) < dminl)
    return ~dropped


def maps(mode, z, c0, lo, hi, dmap, occlusion=None, filled=None, dminl=0):
    """sub = dmap + delta (delta 0 without a winner); sub_filled (if occlusion given) = sub where kept, filled elsewhere."""
    d = np.where(np.asarray(z) >= 0, delta(mode, c0, lo, hi), F32(0)).astype(F32)
    sub = (np.asarray(dmap, F32) + d).astype(F32)
    if occlusion is None:
        return sub, None
    return sub, np.where(kept(occlusion, dminl), sub, np.asarray(filled, F32)).astype(F32)


def brute_state(q, ranges, chunk=1):
    """The kernels' state machine (smx_common.h WtaRunNbr + nbr_merge) per pixel, over calls on `ranges`
    [(s0, s1), ...] (the first fresh) in chunks of `chunk` slices.  -> (z, lo, hi, last) like winners()."""
    q = np.asarray(q, F32)
    D, h, w = q.shape
    Z = np.full((h, w), -1, np.int64)
    LO = np.full((h, w), NAN, F32)
    HI = np.full((h, w), NAN, F32)
    LAST = np.full((h, w), NAN, F32)
    for y in range(h):
        for x in range(w):
            kz, kc = -1, None                # incoming key: winner slice and cost (-1: identity)
            lo = hi = last = NAN
            for s_begin, s_end in ranges:
                for c0 in range(s_begin, s_end, chunk):
                    c1 = min(s_end, c0 + chunk)
                    m, rz = F32(np.inf), -1
                    rlo, rhi = NAN, NAN
                    prev = last if kz >= 0 else NAN
                    for s in range(c0, c1):
                        v = q[s, y, x]
                        take = bool(v <= m)
                        h1 = v if rz + 1 == s and rz >= 0 else rhi
                        rlo = prev if take else rlo
                        rhi = NAN if take else h1
                        if take:
                            m, rz = v, s
                        prev = v
                    run_wins = rz >= 0 and (kz < 0 or m < kc or (m == kc and rz > kz))
                    if run_wins:
                        kz, kc, lo, hi = rz, m, rlo, rhi
                    elif kz < 0:
                        lo = hi = NAN
                    elif kz + 1 == c0:
                        hi = q[c0, y, x]
                    last = prev
            Z[y, x], LO[y, x], HI[y, x], LAST[y, x] = kz, lo, hi, last
    return Z, LO, HI, LAST
