"""numpy reference of the information permeability filter (include/smx.h, above smx_perm_params; Cigla & Alatan 2013): the
weight table, the permeabilities of a guide, the four recurrences of a volume and its winners.  Nothing is imported from the
library; float32 throughout, every product and every sum rounded on its own, so the kernels' results equal these bit for bit.
"""
import math

import numpy as np

F32 = np.float32
DEFAULT_SIGMA = 32.0


def table(sigma):
    """t[k] = (float)exp(-k / sigma), k = 0 .. 255, in double (math.exp is the C library's exp, as in the library's host code)"""
    return np.array([math.exp(-float(k) / float(sigma)) for k in range(256)], np.float64).astype(F32)


def _diff(a, b):
    """|a - b| per pixel: one channel as it is, 3 or 4 channels the maximum over R, G, B (alpha is ignored)"""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return d if d.ndim == 2 else d[:, :, :3].max(axis=2)


def weights(guide, sigma):
    """guide u8 (h, w) or (h, w, 1 | 3 | 4) -> (mu_h, mu_v) float32 (h, w): mu_h[y][x] belongs to the step from x-1 to x (column
    0 is 0 and unused), mu_v[y][x] to the step from y-1 to y (row 0 likewise)"""
    g = np.asarray(guide)
    assert g.dtype == np.uint8 and g.ndim in (2, 3)
    if g.ndim == 3 and g.shape[2] == 1:
        g = g[:, :, 0]
    t = table(sigma)
    h, w = g.shape[:2]
    mu_h, mu_v = np.zeros((h, w), F32), np.zeros((h, w), F32)
    mu_h[:, 1:] = t[_diff(g[:, 1:], g[:, :-1])]
    mu_v[1:, :] = t[_diff(g[1:], g[:-1])]
    return mu_h, mu_v


def _pass_x(c, mu):
    """the three lines of the definition along the last axis of c (..., w) with mu (..., w) broadcast against it"""
    w = c.shape[-1]
    lr, rl = np.empty_like(c), np.empty_like(c)
    lr[..., 0] = c[..., 0]
    for x in range(1, w):
        lr[..., x] = c[..., x] + (mu[..., x] * lr[..., x - 1]).astype(F32)
    rl[..., w - 1] = c[..., w - 1]
    for x in range(w - 2, -1, -1):
        rl[..., x] = c[..., x] + (mu[..., x + 1] * rl[..., x + 1]).astype(F32)
    return ((lr + rl).astype(F32) - c).astype(F32)


def filter_volume(vol, guide, sigma=DEFAULT_SIGMA):
    """vol float32 (D, h, w) -> out (D, h, w): the horizontal pass on every row with mu_h, then the vertical pass on every column
    of its result with mu_v"""
    c = np.ascontiguousarray(vol, F32)
    assert c.ndim == 3
    mu_h, mu_v = weights(guide, sigma)
    with np.errstate(all="ignore"):
        hh = _pass_x(c, mu_h[None])
        out = _pass_x(np.ascontiguousarray(hh.transpose(0, 2, 1)), np.ascontiguousarray(mu_v.T)[None])
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def filter_volume_loops(vol, guide, sigma=DEFAULT_SIGMA):
    """the same definition pixel by pixel on Python scalars of float32 (for small shapes)"""
    c = np.asarray(vol, F32)
    D, h, w = c.shape
    mu_h, mu_v = weights(guide, sigma)
    out = np.empty_like(c)
    with np.errstate(all="ignore"):
        for z in range(D):
            hh = np.empty((h, w), F32)
            for y in range(h):
                lr, rl = [None] * w, [None] * w
                lr[0] = c[z, y, 0]
                for x in range(1, w):
                    lr[x] = F32(c[z, y, x] + F32(mu_h[y, x] * lr[x - 1]))
                rl[w - 1] = c[z, y, w - 1]
                for x in range(w - 2, -1, -1):
                    rl[x] = F32(c[z, y, x] + F32(mu_h[y, x + 1] * rl[x + 1]))
                for x in range(w):
                    hh[y, x] = F32(F32(lr[x] + rl[x]) - c[z, y, x])
            for x in range(w):
                tb, bt = [None] * h, [None] * h
                tb[0] = hh[0, x]
                for y in range(1, h):
                    tb[y] = F32(hh[y, x] + F32(mu_v[y, x] * tb[y - 1]))
                bt[h - 1] = hh[h - 1, x]
                for y in range(h - 2, -1, -1):
                    bt[y] = F32(hh[y, x] + F32(mu_v[y + 1, x] * bt[y + 1]))
                for y in range(h):
                    out[z, y, x] = F32(F32(tb[y] + bt[y]) - hh[y, x])
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
    return np.where(np.asarray(z) >= 0, k.view(np.int64), np.iinfo(np.int64).max)


def label_map(z, dmin):
    """dmin + winning slice as float32 (dmin where there is no winner, as the host entry unpacks the identity key)"""
    return (int(dmin) + np.maximum(z, 0)).astype(F32)
