"""numpy reference of hierarchical min-sum belief propagation as include/smx.h defines it (the contract above smx_bp_params:
Felzenszwalb and Huttenlocher's truncated-linear messages, checkerboard schedule and pyramid).  Vectorised over the pixels,
with the min-convolution as the two-pass distance transform.  A helper module imported by name (tests/test_bp_cpu.py holds
it against a scalar brute force; tests/test_gpu_bp.py holds the kernels against it, bit for bit).

Messages of a level: M[k][z][y][x], k = 0 from the left neighbour, 1 from the right, 2 from the upper, 3 from the lower one.
"""
import numpy as np

import uniq_ref

F32 = np.float32
# (dx, dy) of the neighbour a message of slot k comes FROM, and the slot of the opposite direction
FROM = ((-1, 0), (1, 0), (0, -1), (0, 1))
OPPOSITE = (1, 0, 3, 2)


def clamp(cost, data_scale=1.0):
    """The integer a cost value is read as: t = c * data_scale in f32, C = t >= 0 ? (t <= 255 ? (int)t : 255) : 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(cost, F32) * F32(data_scale)).astype(F32)
        ok = t >= 0
        small = np.where(ok & (t <= 255), t, F32(0)).astype(np.int32)
        return np.where(ok, np.where(t <= 255, small, 255), 0).astype(np.int32)


def pyramid(C, levels):
    """[D_0 .. D_{levels-1}], int64 [z][y][x]: a coarse cell sums its up to four children."""
    out = [np.asarray(C, np.int64)]
    for _ in range(levels - 1):
        f = out[-1]
        D, h, w = f.shape
        pad = np.zeros((D, (h + 1) // 2 * 2, (w + 1) // 2 * 2), np.int64)
        pad[:, :h, :w] = f
        out.append(pad[:, 0::2, 0::2] + pad[:, 0::2, 1::2] + pad[:, 1::2, 0::2] + pad[:, 1::2, 1::2])
    return out


def message(hv, step, trunc):
    """The normalised message of h [z][...]: m'(z) = min_z' (h(z') + min(step |z - z'|, trunc)), m = m' - min m'."""
    f = np.array(hv, np.int64)
    for z in range(1, f.shape[0]):
        np.minimum(f[z], f[z - 1] + step, out=f[z])
    for z in range(f.shape[0] - 2, -1, -1):
        np.minimum(f[z], f[z + 1] + step, out=f[z])
    np.minimum(f, hv.min(axis=0)[None] + trunc, out=f)
    return f - f.min(axis=0)[None]


def _shift(a, dx, dy):
    """out[.., y, x] = a[.., y + dy, x + dx] where that lies inside (0 elsewhere)"""
    out = np.zeros_like(a)
    h, w = a.shape[-2:]
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[..., yd, xd] = a[..., ys, xs]
    return out


def iterate(Dl, M, step, trunc, iterations):
    """`iterations` checkerboard iterations on one level, in place on M [4][z][y][x]."""
    _, h, w = Dl.shape
    yy, xx = np.mgrid[0:h, 0:w]
    for t in range(1, iterations + 1):
        tot = Dl + M.sum(axis=0)
        new = []
        for k, (dx, dy) in enumerate(FROM):
            # what every pixel q would send to its neighbour in the direction (-dx, -dy): all but what came from there
            sent = message(tot - M[OPPOSITE[k]], step, trunc)
            inside = (xx + dx >= 0) & (xx + dx < w) & (yy + dy >= 0) & (yy + dy < h)
            new.append((_shift(sent, dx, dy), inside & ((xx + yy + t) % 2 == 0)))
        for k, (val, mask) in enumerate(new):
            M[k] = np.where(mask[None], val, M[k])
    return M


def run(C, step=20, trunc=60, iterations=5, levels=4, trace=None):
    """S [z][y][x] int64 of an integer volume C.  trace (a list) receives (level, M) after each level's iterations."""
    pyr = pyramid(C, levels)
    M = np.zeros((4,) + pyr[-1].shape, np.int64)
    for l in range(levels - 1, -1, -1):
        Dl = pyr[l]
        if l < levels - 1:
            _, h, w = Dl.shape
            M = M[:, :, np.arange(h) >> 1][:, :, :, np.arange(w) >> 1].copy()
        iterate(Dl, M, step, trunc, iterations)
        if trace is not None:
            trace.append((l, M.copy()))
    return pyr[0] + M.sum(axis=0)


def aggregate(cost, step=20, trunc=60, iterations=5, levels=4, data_scale=1.0):
    return run(clamp(cost, data_scale), step, trunc, iterations, levels).astype(np.int32)


def winners(S):
    """z* per pixel: the LARGEST z of minimal S."""
    D = S.shape[0]
    return (D - 1 - np.argmin(S[::-1], axis=0)).astype(np.int64)


def pack_keys(costs, z):
    """smx_pack_key for non-negative finite costs: the f32 bits << 32 | (0xFFFFFFFF - z), as int64."""
    u = np.asarray(costs, F32).view(np.uint32).astype(np.uint64)
    return ((u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - z.astype(np.uint64))).view(np.int64)


def outputs(cost, step=20, trunc=60, iterations=5, levels=4, data_scale=1.0):
    """What one view of smx_dev_bp_wta_pair writes: keys (h, w) int64, agg (D, h, w) float32, nbr (3, h, w) float32 (lo, hi,
    last), uq (3, h, w) float32 (sec, rest, last), and z, S, best for the tests' own use."""
    S = aggregate(cost, step, trunc, iterations, levels, data_scale)
    D = S.shape[0]
    z = winners(S)
    agg = S.astype(F32)
    best = np.take_along_axis(agg, z[None], axis=0)[0]
    nan = F32(np.nan)
    lo = np.where(z > 0, np.take_along_axis(agg, np.maximum(z - 1, 0)[None], axis=0)[0], nan).astype(F32)
    hi = np.where(z < D - 1, np.take_along_axis(agg, np.minimum(z + 1, D - 1)[None], axis=0)[0], nan).astype(F32)
    _, _, sec, rest, last, _ = uniq_ref.second_best(agg)
    return {"keys": pack_keys(best, z), "agg": agg, "nbr": np.stack((lo, hi, agg[D - 1])), "uq": np.stack((sec, rest, last)),
            "z": z, "S": S, "best": best}
