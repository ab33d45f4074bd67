"""numpy reference of the AD-Census matching cost, written from the definition of include/smx.h (smx_adcensus_params), not
from the kernel.  The census half is tests/census_ref.py.

  tables (double, nch = 3 if colour else 1):
      T[k]      = float32(scale * (1.0 - exp(-k / lambda_census)))        k = 0 .. 63
      T[64 + s] = float32(scale * (1.0 - exp(-s / (nch * lambda_ad))))    s = 0 .. 765
  cost[z][y][x] = T[min(popcount(own_code[y][x] ^ other_code[y][x + d]), t)] + T[64 + sum_c |own_c[y][x] - other_c[y][x + d]|]
      if 0 <= x + d < w else T[t] + T[64 + 255 nch];  d = dmin + z, t = min(th, nbits); one float32 addition.
  The images: (h, w) uint8, or (h, w, 3 or 4) uint8 of which R, G, B are read; the codes come from gray images.
"""
import numpy as np

import census_ref

DEFAULTS = dict(rx=4, ry=3, th=62, lambda_census=30.0, lambda_ad=10.0, scale=127.5, colour=0)
TABLE_FLOATS = 64 + 766


def tables(lambda_census=30.0, lambda_ad=10.0, scale=127.5, colour=0):
    nch = 3 if colour else 1
    k = np.arange(64, dtype=np.float64)
    s = np.arange(766, dtype=np.float64)
    tc = np.float64(scale) * (1.0 - np.exp(-k / np.float64(lambda_census)))
    ta = np.float64(scale) * (1.0 - np.exp(-s / (np.float64(nch) * np.float64(lambda_ad))))
    return np.concatenate([tc, ta]).astype(np.float32)


def cost(own, other, own_gray, other_gray, size_d, dmin, rx=4, ry=3, th=62, lambda_census=30.0, lambda_ad=10.0, scale=127.5,
         colour=0, s_begin=0, s_end=None, table=None):
    """Slices [s_begin, s_end) of the volume of `own` against `other`.  own / other: the images of the AD term, (h, w) with
    colour 0, (h, w, 3 or 4) with colour 1; own_gray / other_gray: the gray images of the codes (with colour 0 the same
    arrays).  table: the tables to use instead of tables(...) (e.g. the library's)."""
    T = tables(lambda_census, lambda_ad, scale, colour) if table is None else np.asarray(table, np.float32)
    assert T.shape == (TABLE_FLOATS,)
    nch = 3 if colour else 1
    a = np.asarray(own, np.uint8).astype(np.int64)
    b = np.asarray(other, np.uint8).astype(np.int64)
    if colour:
        assert a.ndim == 3 and a.shape[2] in (3, 4)
        a, b = a[..., :3], b[..., :3]
    else:
        assert a.ndim == 2
        a, b = a[..., None], b[..., None]
    co, cx = census_ref.census_transform(own_gray, rx, ry), census_ref.census_transform(other_gray, rx, ry)
    h, w = co.shape
    s_end = size_d if s_end is None else s_end
    t = min(th, census_ref.nbits(rx, ry))
    out = np.full((s_end - s_begin, h, w), T[t] + T[64 + 255 * nch], np.float32)
    for z in range(s_begin, s_end):
        d = dmin + z
        x0, x1 = max(0, -d), min(w, w - d)           # the x with 0 <= x + d < w
        if x0 < x1:
            hc = np.minimum(census_ref.popcount(co[:, x0:x1] ^ cx[:, x0 + d:x1 + d]), t)
            s = np.abs(a[:, x0:x1] - b[:, x0 + d:x1 + d]).sum(axis=-1)
            out[z - s_begin, :, x0:x1] = T[hc] + T[64 + s]
    return out


def gray_cost(i1, i2, size_d, dmin, **kw):
    """colour 0: the AD term and the codes from the same gray images."""
    return cost(i1, i2, i1, i2, size_d, dmin, colour=0, **kw)
