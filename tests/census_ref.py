"""numpy reference of the census transform and its Hamming cost, written from the definitions of include/smx.h
(smx_census_params), not from the kernels.

  code(y, x): the window's neighbours are numbered k = 0, 1, ... with dy = -ry .. ry outside, dx = -rx .. rx inside, the
              centre skipped; bit k (bit 0 = LSB) is set iff I[clamp(y + dy)][clamp(x + dx)] < I[y][x] (replicate clamp).
  cost[z][y][x] = min(popcount(own[y][x] ^ other[y][x + d]), t) if 0 <= x + d < w else t, d = dmin + z,
              t = min(th, nbits), nbits = (2 rx + 1)(2 ry + 1) - 1; float32.
"""
import numpy as np

DEFAULTS = (4, 3, 62)        # rx, ry, th


def nbits(rx, ry):
    return (2 * rx + 1) * (2 * ry + 1) - 1


def popcount(a):
    """Set bits of every element of a uint64 array (as int64 counts)."""
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int64)


def census_transform(img, rx=4, ry=3):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    ys, xs = np.arange(h), np.arange(w)
    code = np.zeros((h, w), np.uint64)
    k = 0
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            if dy == 0 and dx == 0:
                continue
            nb = img[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
            code |= (nb < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return code


def cost_from_codes(own, other, size_d, dmin, rx=4, ry=3, th=62, s_begin=0, s_end=None):
    """Slices [s_begin, s_end) of the volume of `own` against `other`."""
    h, w = own.shape
    s_end = size_d if s_end is None else s_end
    t = min(th, nbits(rx, ry))
    cost = np.full((s_end - s_begin, h, w), np.float32(t), np.float32)
    for z in range(s_begin, s_end):
        d = dmin + z
        x0, x1 = max(0, -d), min(w, w - d)           # the x with 0 <= x + d < w
        if x0 < x1:
            ham = popcount(own[:, x0:x1] ^ other[:, x0 + d:x1 + d])
            cost[z - s_begin, :, x0:x1] = np.minimum(ham, t).astype(np.float32)
    return cost


def census_cost(i1, i2, size_d, dmin, rx=4, ry=3, th=62, s_begin=0, s_end=None):
    return cost_from_codes(census_transform(i1, rx, ry), census_transform(i2, rx, ry), size_d, dmin, rx, ry, th,
                           s_begin, s_end)
