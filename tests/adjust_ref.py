"""numpy reference of the depth-discontinuity adjustment as include/smx.h defines it (smx_dev_discontinuity_adjust): integers
and float32 comparisons, and the one float32 formula of the sub-pixel map (subpix_ref.delta).  A plain helper module, imported by
name: tests/test_adjust_cpu.py holds it against a scalar brute force; tests/test_gpu_adjust.py holds the kernel against it, bit
for bit.
"""
import numpy as np

import subpix_ref

F32 = np.float32
DEFAULTS = dict(tau_e=2, vertical=1, iterations=1)
MAX_D = 512
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1))         # (dx, dy), the order of the candidates; the last two with vertical


def params_ok(tau_e, vertical, iterations):
    return 1 <= tau_e <= 512 and vertical in (0, 1) and 1 <= iterations <= 8


def shape_ok(w, h, size_d):
    return w >= 1 and h >= 1 and w * h < 2 ** 31 and 1 <= size_d <= MAX_D


def labelled(disp, dmin, size_d):
    """(mask, z): a pixel is labelled iff its value is finite, integer-valued and 0 <= value - dmin < size_d; z = value - dmin
    (int64, 0 where not labelled)"""
    d = np.ascontiguousarray(disp, F32)
    fin = np.isfinite(d)
    t = np.where(fin, d, 0).astype(np.float64)
    whole = fin & (t == np.trunc(t))
    z = np.where(whole, t, 0.0) - float(int(dmin))      # (exact below 2^53; beyond it z is far out of range either way)
    ok = whole & (z >= 0) & (z < size_d)
    return ok, np.where(ok, z, 0).astype(np.int64)


def _shift(a, dx, dy, fill):
    """b[y][x] = a[y + dy][x + dx], `fill` outside the image"""
    h, w = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def adjust_round(disp, vol, dmin, tau_e, vertical, stats=None):
    """M_{k+1} from M_k: one Jacobi round.  -> (map, own cost after the round where labelled else NaN).  stats (a dict) collects
    the counts of discontinuity pixels that changed / stayed, by the axis of the winning / of any candidate"""
    d = np.ascontiguousarray(disp, F32)
    vol = np.asarray(vol, F32)
    size_d = vol.shape[0]
    lab, z = labelled(d, dmin, size_d)
    bits = d.view(np.uint32).copy()
    best = np.take_along_axis(vol, z[None], 0)[0].copy()
    has = np.zeros(d.shape, bool)
    has_axis = [np.zeros(d.shape, bool), np.zeros(d.shape, bool)]
    won = np.full(d.shape, -1)
    for i, (dx, dy) in enumerate(NEIGHBOURS[:4 if vertical else 2]):
        qlab = _shift(lab, dx, dy, False)
        qz = _shift(z, dx, dy, 0)
        qbits = _shift(d.view(np.uint32), dx, dy, 0)
        cand = lab & qlab & (np.abs(qz - z) >= tau_e)
        cost = np.take_along_axis(vol, np.where(cand, qz, 0)[None], 0)[0]
        with np.errstate(invalid="ignore"):
            take = cand & (cost < best)
        best = np.where(take, cost, best)
        bits = np.where(take, qbits, bits)
        won = np.where(take, i, won)
        has |= cand
        has_axis[i // 2] |= cand
    if stats is not None:
        for k, m in (("changed", won >= 0), ("unchanged", has & (won < 0)), ("changed_h", (won == 0) | (won == 1)),
                     ("changed_v", won >= 2), ("candidate_h", has_axis[0]), ("candidate_v", has_axis[1])):
            stats[k] = stats.get(k, 0) + int(m.sum())
    return bits.view(F32), np.where(lab, best, F32(np.nan)).astype(F32)


def adjust(disp, vol, dmin, tau_e=2, vertical=1, iterations=1, mode=None, sub=None, stats=None, rounds=None):
    """The whole call.  -> the map, or (map, sub) with mode (subpix_ref.PARABOLA / EQUIANGULAR) and sub given.  rounds (a list)
    receives the map after every round."""
    vol = np.asarray(vol, F32)
    size_d = vol.shape[0]
    if not params_ok(tau_e, vertical, iterations) or not shape_ok(np.shape(disp)[1], np.shape(disp)[0], size_d):
        raise ValueError("invalid parameters")
    d0 = np.ascontiguousarray(disp, F32)
    cur = d0
    for _ in range(iterations):
        cur, _ = adjust_round(cur, vol, dmin, tau_e, vertical, stats)
        if rounds is not None:
            rounds.append(cur.copy())
    if sub is None:
        return cur
    _, z0 = labelled(d0, dmin, size_d)
    _, z1 = labelled(cur, dmin, size_d)
    changed = z0 != z1                              # (a changed pixel was and stays labelled)
    c0 = np.take_along_axis(vol, z1[None], 0)[0]
    lo = np.where(z1 > 0, np.take_along_axis(vol, np.maximum(z1 - 1, 0)[None], 0)[0], subpix_ref.NAN)
    hi = np.where(z1 + 1 < size_d, np.take_along_axis(vol, np.minimum(z1 + 1, size_d - 1)[None], 0)[0], subpix_ref.NAN)
    with np.errstate(all="ignore"):                 # (unlabelled pixels hold anything; they are not taken)
        fit = (cur + subpix_ref.delta(mode, c0, lo, hi)).astype(F32)
    s = np.ascontiguousarray(sub, F32)
    out = np.where(changed, fit.view(np.uint32), s.view(np.uint32)).view(F32)
    return cur, out


def own_cost(disp, vol, dmin):
    """A[z(p)][p] where p is labelled, NaN elsewhere"""
    vol = np.asarray(vol, F32)
    lab, z = labelled(disp, dmin, vol.shape[0])
    return np.where(lab, np.take_along_axis(vol, z[None], 0)[0], F32(np.nan)).astype(F32)


def brute(disp, vol, dmin, tau_e=2, vertical=1, iterations=1, mode=None, sub=None):
    """The definition pixel by pixel, in python scalars"""
    vol = np.asarray(vol, F32)
    size_d, h, w = vol.shape
    cur = np.ascontiguousarray(disp, F32).copy()
    s = None if sub is None else np.ascontiguousarray(sub, F32).copy()

    def slice_of(v):
        v = float(v)
        if v != v or v in (float("inf"), float("-inf")) or v != int(v):
            return -1
        zz = int(v) - int(dmin)
        return zz if 0 <= zz < size_d else -1

    first = [[slice_of(cur[y, x]) for x in range(w)] for y in range(h)]
    for _ in range(iterations):
        nxt = cur.copy()
        for y in range(h):
            for x in range(w):
                zp = slice_of(cur[y, x])
                if zp < 0:
                    continue
                best = vol[zp, y, x]
                for dx, dy in NEIGHBOURS[:4 if vertical else 2]:
                    qx, qy = x + dx, y + dy
                    if not (0 <= qx < w and 0 <= qy < h):
                        continue
                    zq = slice_of(cur[qy, qx])
                    if zq < 0 or abs(zq - zp) < tau_e:
                        continue
                    if vol[zq, y, x] < best:
                        best = vol[zq, y, x]
                        nxt[y, x] = cur[qy, qx]
        cur = nxt
    if s is None:
        return cur
    for y in range(h):
        for x in range(w):
            z1 = slice_of(cur[y, x])
            if z1 == first[y][x]:
                continue
            lo = vol[z1 - 1, y, x] if z1 > 0 else subpix_ref.NAN
            hi = vol[z1 + 1, y, x] if z1 + 1 < size_d else subpix_ref.NAN
            s[y, x] = cur[y, x] + subpix_ref.delta(mode, vol[z1, y, x], lo, hi)
    return cur, s
