"""numpy reference of the scan-line optimiser with colour-adaptive penalties as include/smx.h defines it
(smx_dev_scanline_wta_pair): tests/sgm_ref.py with penalties per pixel, direction and label.  Vectorised over the labels and
over a row, a plain loop along each path.  A helper module imported by name (tests/test_scanline_cpu.py holds it against a
scalar brute force; tests/test_gpu_scanline.py holds the kernels against it, bit for bit).
"""
import numpy as np

import sgm_ref
from sgm_ref import BIG, DIRS8, clamp, directions, pack_keys, winners  # noqa: F401  (re-exported for the tests)

DEFAULTS = dict(p1=127, p2=382, tau_so=15, paths=4)
DIV = (1, 4, 10)


def params_ok(p1, p2, tau_so, paths):
    return 0 <= p1 <= p2 <= 4095 and 1 <= tau_so <= 256 and paths in (4, 8)


def _channels(guide):
    """(h, w, 1 or 3) int32: the bytes the colour distance reads (a fourth byte is ignored)"""
    g = np.asarray(guide)
    assert g.dtype == np.uint8 and g.ndim in (2, 3)
    if g.ndim == 2:
        g = g[:, :, None]
    assert g.shape[2] in (1, 3, 4)
    return g[:, :, :3].astype(np.int32)


def edges(guide, dx, dy, tau_so):
    """(h, w) bool: e(p, r) = [D(p, p - r) >= tau_so], False where p - r lies outside the image"""
    I = _channels(guide)
    h, w = I.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    qy, qx = yy - dy, xx - dx
    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    D = np.abs(I - I[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)]).max(axis=2)
    return inside & (D >= tau_so)


def edge_count(guide_own, guide_other, dx, dy, dmin, size_d, tau_so):
    """k = e1 + e2, (size_d, h, w) int: the partner of (x, y) at slice z is (x + dmin + z, y) in the other view; e2 is 0 where
    the partner or its predecessor lies outside the image"""
    e1 = edges(guide_own, dx, dy, tau_so)
    eo = edges(guide_other, dx, dy, tau_so)          # already False where the predecessor is outside
    h, w = e1.shape
    x = np.arange(w)
    k = np.empty((size_d, h, w), np.int64)
    for z in range(size_d):
        xq = x + dmin + z
        ok = (xq >= 0) & (xq < w)
        e2 = eo[:, np.clip(xq, 0, w - 1)] & ok[None, :]
        k[z] = e1.astype(np.int64) + e2
    return k


def path_costs(C, k, dx, dy, p1, p2):
    """L_r of the direction (dx, dy) for an integer volume C [z][y][x] and the edge counts k [z][y][x] -> int32"""
    if dy == 0:         # a horizontal path is a vertical one of the transposed image
        return path_costs(C.transpose(0, 2, 1), k.transpose(0, 2, 1), 0, dx, p1, p2).transpose(0, 2, 1)
    D, h, w = C.shape
    P1 = np.array([p1 // d for d in DIV], np.int64)[k]
    P2 = np.array([p2 // d for d in DIV], np.int64)[k]
    L = np.empty((D, h, w), np.int64)
    x = np.arange(w)
    inside = (x - dx >= 0) & (x - dx < w)
    src = np.clip(x - dx, 0, w - 1)
    pad = np.full((1, w), BIG, np.int64)
    for i in range(h):
        y = i if dy > 0 else h - 1 - i
        if i == 0:
            L[:, y] = C[:, y]
            continue
        prev = L[:, y - dy][:, src]
        m = prev.min(axis=0)
        lo = np.concatenate((pad, prev[:-1])) + P1[:, y]
        hi = np.concatenate((prev[1:], pad)) + P1[:, y]
        step = C[:, y] + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + P2[:, y])) - m
        L[:, y] = np.where(inside, step, C[:, y])
    return L.astype(np.int32)


def aggregate(guide_own, guide_other, cost, dmin=0, p1=127, p2=382, tau_so=15, paths=4):
    """S [z][y][x] int32 of one view's cost volume of any float values"""
    assert params_ok(p1, p2, tau_so, paths)
    C = clamp(cost)
    S = np.zeros(C.shape, np.int32)
    for dx, dy in directions(paths):
        k = edge_count(guide_own, guide_other, dx, dy, dmin, C.shape[0], tau_so)
        S += path_costs(C, k, dx, dy, p1, p2)
    return S


def outputs_of(S):
    """What one view of the device entry writes for the sums S: the dict of sgm_ref.outputs"""
    D, h, w = S.shape
    z = winners(S)
    agg = S.astype(np.float32)
    best = np.take_along_axis(agg, z[None], axis=0)[0]
    nan = np.float32(np.nan)
    lo = np.where(z > 0, np.take_along_axis(agg, np.maximum(z - 1, 0)[None], axis=0)[0], nan).astype(np.float32)
    hi = np.where(z < D - 1, np.take_along_axis(agg, np.minimum(z + 1, D - 1)[None], axis=0)[0], nan).astype(np.float32)
    return {"keys": pack_keys(best, z), "agg": agg, "nbr": np.stack((lo, hi, agg[D - 1])), "z": z, "S": S, "best": best}


def outputs(guide_own, guide_other, cost, dmin=0, **kw):
    return outputs_of(aggregate(guide_own, guide_other, cost, dmin, **kw))


def thin_scene(seed=7, h=24, w=64, D=8, x0=30, sw=3, bg=2, fg=5):
    """A thin foreground strip of another colour in front of a weakly textured surface, with noisy costs: (left guide, right
    guide, cost of the left view, truth).  dmin = 0: the partner of (x, z) is x + z in the right guide."""
    rng = np.random.default_rng(seed)
    gl = np.empty((h, w, 3), np.int32); gl[:] = (150, 60, 60); gl[:, x0:x0 + sw] = (60, 105, 60)
    truth = np.full((h, w), bg, np.int64); truth[:, x0:x0 + sw] = fg
    gr = np.empty((h, w, 3), np.int32); gr[:] = (150, 60, 60); gr[:, x0 + fg:x0 + sw + fg] = (60, 105, 60)
    gl = (gl + rng.integers(-2, 3, gl.shape)).astype(np.uint8)
    gr = (gr + rng.integers(-2, 3, gr.shape)).astype(np.uint8)
    cost = rng.integers(25, 60, (D, h, w)).astype(np.float32)
    np.put_along_axis(cost, truth[None], rng.integers(10, 45, (1, h, w)).astype(np.float32), axis=0)
    return gl, gr, cost, truth
