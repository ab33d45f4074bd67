"""numpy reference of cross-scale cost aggregation (include/smx.h, above smx_cscale_params; Zhang et al., CVPR 2014): the u8
pyramid, a level's geometry, the levels' weights, the combination of the levels' aggregated volumes and its winners.  Nothing is
imported from the library; float32 and integers throughout, so the kernels' results equal these bit for bit.
"""
import numpy as np

F32 = np.float32
IDENT = np.iinfo(np.int64).max
TAPS = np.array([1, 4, 6, 4, 1], np.int64)
MAX_SCALES = 5


def reflect101(i, n):
    """i < 0 -> -i, i >= n -> 2(n-1) - i, then clamped to [0, n-1] (the clamp matters for n of 1 or 2)"""
    i = np.asarray(i, np.int64)
    i = np.where(i < 0, -i, i)
    i = np.where(i >= n, 2 * (n - 1) - i, i)
    return np.clip(i, 0, n - 1)


def pyr_down(img):
    """u8 (h, w) or (h, w, channels) -> ((h+1)//2, (w+1)//2[, channels]): 1 4 6 4 1 along x on integers, then along y on those
    sums, at the even source coordinates, (t + 128) >> 8"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    v = a.astype(np.int64).reshape(a.shape[0], a.shape[1], -1)
    h, w, _ = v.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xs = reflect101(2 * np.arange(wo)[:, None] - 2 + np.arange(5)[None], w)        # [wo][5]
    ys = reflect101(2 * np.arange(ho)[:, None] - 2 + np.arange(5)[None], h)        # [ho][5]
    rows = (v[:, xs, :] * TAPS[None, None, :, None]).sum(axis=2)                    # [h][wo][c]
    t = (rows[ys, :, :] * TAPS[None, :, None, None]).sum(axis=1)                    # [ho][wo][c]
    out = ((t + 128) >> 8).astype(np.uint8)
    return out.reshape((ho, wo) + a.shape[2:])


def pyramid(img, scales):
    """[level 0 .. level scales-1]"""
    out = [np.ascontiguousarray(img)]
    for _ in range(1, scales):
        out.append(pyr_down(out[-1]))
    return out


def level(w, h, dmin, size_d, s):
    """-> (w_s, h_s, dmin_s, size_d_s); >> on Python ints is the arithmetic shift (floor for negative labels)"""
    for _ in range(s):
        w, h = (w + 1) // 2, (h + 1) // 2
    lo, hi = int(dmin) >> s, (int(dmin) + int(size_d) - 1) >> s
    return w, h, lo, hi - lo + 1


def matrix(scales, lam):
    """the regulariser's tridiagonal matrix M, in double"""
    m = np.zeros((scales, scales), np.float64)
    for i in range(scales):
        m[i, i] = 1.0 + lam * ((i > 0) + (i + 1 < scales))
        if i:
            m[i, i - 1] = m[i - 1, i] = -lam
    return m


def weights(scales, lam):
    """wt[s] = (float)(M^-1)[0][s]: M x = e_0 (M is symmetric) by the Thomas elimination on Python floats (IEEE double, each
    operation rounded on its own) -- the recurrence of the library's host code, so the f32 results are the same bits"""
    lam = float(lam)
    off = -lam
    c, r = [0.0] * scales, [0.0] * scales
    for i in range(scales):
        d = 1.0 + lam * float((i > 0) + (i + 1 < scales))
        m = d - off * c[i - 1] if i else d
        c[i] = off / m
        r[i] = (0.0 - off * r[i - 1]) / m if i else 1.0 / m
    x = [0.0] * scales
    x[-1] = r[-1]
    for i in range(scales - 2, -1, -1):
        x[i] = r[i] - c[i] * x[i + 1]
    return np.array(x, np.float64).astype(F32)


def combine(levels, dmin, size_d, lam):
    """levels[s]: A_s (size_d_s, h_s, w_s) float32 -> out (size_d, h, w) float32: out = wt[0] * A_0, then + wt[s] * (A_s at the
    label's and the pixel's ancestors) for s = 1 .. in order, every product and every sum rounded to float32"""
    scales = len(levels)
    a0 = np.asarray(levels[0], F32)
    D, h, w = a0.shape
    assert D == size_d
    wt = weights(scales, lam)
    ys, xs = np.arange(h), np.arange(w)
    lab = int(dmin) + np.arange(D)
    with np.errstate(all="ignore"):
        out = (wt[0] * a0).astype(F32)
        for s in range(1, scales):
            a = np.asarray(levels[s], F32)
            ws, hs, lo, ds = level(w, h, dmin, size_d, s)
            assert a.shape == (ds, hs, ws), (a.shape, (ds, hs, ws))
            t = (wt[s] * a).astype(F32)
            out = (out + t[((lab >> s) - lo)[:, None, None], (ys >> s)[None, :, None], (xs >> s)[None, None, :]]).astype(F32)
    return out


def winners(q):
    """-> (z, c0): the winning slice of q (D, h, w) by the packed key's rule with ascending slices (smallest cost, the LAST slice
    among equal costs, a NaN never; -1: no winner) and its cost with -0 folded to +0"""
    q = np.asarray(q, F32)
    nan = np.isnan(q)
    has = ~nan.all(axis=0)
    m = np.where(nan, F32(np.inf), q).min(axis=0)
    hit = (q == m[None]) & ~nan
    k = q.shape[0] - 1 - np.argmax(hit[::-1], axis=0)
    z = np.where(has, k, -1)
    c0 = np.take_along_axis(q, np.where(has, k, 0)[None], 0)[0]
    return z, np.where(c0 == 0, F32(0), c0).astype(F32)


def pack_keys(z, c0):
    """the packed int64 keys of winners (z, c0); z < 0 gives the identity"""
    c = np.ascontiguousarray(c0, F32)
    u = c.view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), (~u ^ np.uint64(0x80000000)) & np.uint64(0xFFFFFFFF), u)
    k = (u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.maximum(z, 0).astype(np.uint64))
    return np.where(np.asarray(z) >= 0, k.view(np.int64), IDENT)


def label_map(z, dmin):
    """dmin + winning slice as float32 (0 where there is no winner, as the pair's finish leaves it)"""
    return np.where(z >= 0, (int(dmin) + z).astype(F32), F32(0)).astype(F32)
