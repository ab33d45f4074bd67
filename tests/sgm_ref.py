"""numpy reference of semi-global matching as include/smx.h defines it (smx_dev_sgm_wta_pair): vectorised over d, a plain
loop along each path.  A helper module imported by name (tests/test_sgm_cpu.py holds it against a scalar brute force;
tests/test_gpu_sgm.py holds the kernels against it, bit for bit).
"""
import numpy as np

DIRS4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
DIRS8 = DIRS4 + ((1, 1), (-1, 1), (1, -1), (-1, -1))
BIG = 1 << 20


def directions(paths):
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8")
    return DIRS4 if paths == 4 else DIRS8


def clamp(cost):
    """The integer a cost value is read as: C = c >= 0 ? (c <= 255 ? (int)c : 255) : 0 (NaN gives 0)."""
    c = np.asarray(cost, np.float32)
    with np.errstate(invalid="ignore"):
        ok = c >= 0
        small = np.where(ok & (c <= 255), c, np.float32(0)).astype(np.int32)
        return np.where(ok, np.where(c <= 255, small, 255), 0).astype(np.int32)


def path_costs(C, dx, dy, p1, p2):
    """L_r of the direction (dx, dy) for an integer volume C [z][y][x] -> int32 [z][y][x]."""
    if dy == 0:         # a horizontal path is a vertical one of the transposed image
        return path_costs(C.transpose(0, 2, 1), 0, dx, p1, p2).transpose(0, 2, 1)
    D, h, w = C.shape
    L = np.empty((D, h, w), np.int64)
    # all paths of the direction advance one row per step: L[:, y, x] from L[:, y - dy, x - dx]
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
        lo = np.concatenate((pad, prev[:-1])) + p1
        hi = np.concatenate((prev[1:], pad)) + p1
        step = C[:, y] + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + p2)) - m
        L[:, y] = np.where(inside, step, C[:, y])
    return L.astype(np.int32)


def aggregate(cost, p1=10, p2=120, paths=8):
    """S [z][y][x] int32 of a cost volume of any float values."""
    C = clamp(cost)
    S = np.zeros(C.shape, np.int32)
    for dx, dy in directions(paths):
        S += path_costs(C, dx, dy, p1, p2)
    return S


def winners(S):
    """z* per pixel: the LARGEST z of minimal S."""
    D = S.shape[0]
    return (D - 1 - np.argmin(S[::-1], axis=0)).astype(np.int64)


def pack_keys(costs, z):
    """smx_pack_key for non-negative finite costs: the f32 bits << 32 | (0xFFFFFFFF - z), as int64."""
    u = np.asarray(costs, np.float32).view(np.uint32).astype(np.uint64)
    return ((u << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - z.astype(np.uint64))).view(np.int64)


def outputs(cost, p1=10, p2=120, paths=8):
    """What one view of smx_dev_sgm_wta_pair writes: dict keys (h, w) int64, agg (D, h, w) float32, nbr (3, h, w) float32
    (lo, hi, last), and z (h, w), S (D, h, w) int32 for the tests' own use."""
    S = aggregate(cost, p1, p2, paths)
    D, h, w = S.shape
    z = winners(S)
    agg = S.astype(np.float32)
    best = np.take_along_axis(agg, z[None], axis=0)[0]
    nan = np.float32(np.nan)
    lo = np.where(z > 0, np.take_along_axis(agg, np.maximum(z - 1, 0)[None], axis=0)[0], nan).astype(np.float32)
    hi = np.where(z < D - 1, np.take_along_axis(agg, np.minimum(z + 1, D - 1)[None], axis=0)[0], nan).astype(np.float32)
    return {"keys": pack_keys(best, z), "agg": agg, "nbr": np.stack((lo, hi, agg[D - 1])), "z": z, "S": S, "best": best}
