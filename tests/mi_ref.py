"""The mutual-information matching cost in numpy: the definition of include/smx.h ("Mutual-information matching cost"), which
the kernels of smx_mi.hip, smx_mi_table and the context's loop are held to bit for bit.

The table is computed in float64 with every operation rounded on its own and the sums in the order smx.h states; the logarithms
come from math.log, element by element -- the C library's log, the one smx_mi_table calls -- so tables are compared for
equality.  pair_loop is the loop of smx_ctx_set_mi with the aggregation passed in as a function of the two volumes.
"""
import math

import numpy as np

import patchmatch_ref

F32 = np.float32
LEVELS = 256
G = np.array([1, 6, 15, 20, 15, 6, 1], np.float64) / 64.0
INIT_RANDOM, INIT_REFERENCE = 0, 1
BORDER = F32(255.0)


def histogram(img_l, img_r, disp, mark):
    """H[L[y][x]][R[y][x + d]] over the pixels whose label d is not `mark` and whose partner lies inside the image."""
    h, w = img_l.shape
    d = np.asarray(disp, F32)
    xx = np.arange(w, dtype=np.int64)[None, :] + d.astype(np.int64)
    ok = (d != F32(mark)) & (xx >= 0) & (xx < w)
    ys, xs = np.nonzero(ok)
    H = np.zeros((LEVELS, LEVELS), np.uint32)
    np.add.at(H, (img_l[ys, xs], img_r[ys, xx[ys, xs]]), 1)
    return H


def _conv(v, axis):
    """sum over t = 0 .. 6, ascending from 0.0, of g[t] * v[j + t - 3] along `axis`, v taken as 0.0 outside."""
    v = np.moveaxis(np.asarray(v, np.float64), axis, -1)
    pad = np.zeros(v.shape[:-1] + (LEVELS + 6,), np.float64)
    pad[..., 3:3 + LEVELS] = v
    s = np.zeros_like(v)
    for t in range(7):
        s = s + G[t] * pad[..., t:t + LEVELS]
    return np.moveaxis(s, -1, axis)


def _conv2(m):
    return _conv(_conv(m, 1), 0)


def _neg_log(m):
    flat = np.maximum(m, 1e-12).ravel()
    return np.array([-math.log(x) for x in flat], np.float64).reshape(m.shape)


def table(hist):
    """T, uint8 [256][256], of a joint histogram."""
    hist = np.asarray(hist, np.uint32)
    n = int(hist.astype(np.uint64).sum())
    T = np.zeros((LEVELS, LEVELS), np.uint8)
    if n == 0:
        return T
    P = hist.astype(np.float64) / float(n)
    p1 = np.zeros(LEVELS, np.float64)
    p2 = np.zeros(LEVELS, np.float64)
    for k in range(LEVELS):          # ascending, one addition at a time (np.sum adds pairwise)
        p1 = p1 + P[:, k]
        p2 = p2 + P[k, :]
    h12 = _conv2(_neg_log(_conv2(P)))
    h1 = _conv(_neg_log(_conv(p1, 0)), 0)
    h2 = _conv(_neg_log(_conv(p2, 0)), 0)
    c = (h12 - h1[:, None]) - h2[None, :]
    c = c - c.min()
    m = c.max()
    if m == 0.0:
        return T
    return np.rint((c * 255.0) / m).astype(np.uint8)


def cost(T, img_l, img_r, size_d, dmin, right=False, s_begin=0, s_end=None):
    """The volume of one view, float32 [z][y][x] for the slices [s_begin, s_end): the left view's is T[L[y][x]][R[y][xx]], the
    right view's T[L[y][xx]][R[y][x]], xx = x + dmin + z, and 255 where xx lies outside the image."""
    h, w = img_l.shape
    s_end = size_d if s_end is None else s_end
    out = np.full((max(s_end - s_begin, 0), h, w), BORDER, F32)
    x = np.arange(w, dtype=np.int64)
    for z in range(s_begin, s_end):
        xx = x + dmin + z
        ok = (xx >= 0) & (xx < w)
        xs, xo = x[ok], xx[ok]
        if right:
            out[z - s_begin][:, xs] = T[img_l[:, xo], img_r[:, xs]].astype(F32)
        else:
            out[z - s_begin][:, xs] = T[img_l[:, xs], img_r[:, xo]].astype(F32)
    return out


def random_map(w, h, dmin, size_d, seed):
    """dmin + hash(seed, y*w + x) mod size_d, the hash being PatchMatch stereo's with view 0 and draw 0."""
    pix = np.arange(w * h, dtype=np.uint32)
    hs = patchmatch_ref.pm_hash(np.uint32(seed & 0xFFFFFFFF), np.uint32(0), pix, np.uint32(0)).astype(np.uint32)
    return (dmin + (hs % np.uint32(size_d)).astype(np.int64)).astype(F32).reshape(h, w)


def pair_loop(img_l, img_r, size_d, dminl, dminr, solve, iterations=3, init=INIT_RANDOM, seed=0, reference_costs=None):
    """The loop of smx_ctx_set_mi.  solve(cost_l, cost_r) -> dict with at least "occlusion", the LR-checked left map (mark
    dminl - 100): cost volumes -> aggregation -> winners -> LR check (-> fill), the stages behind left out.
    reference_costs() -> (cost_l, cost_r) of the reference's cost, for init = INIT_REFERENCE.
    Returns the list of what solve returned for tables 1 .. iterations, each with "table" and "hist" added."""
    h, w = img_l.shape
    mark = F32(dminl - 100)
    if init == INIT_REFERENCE:
        current = solve(*reference_costs())["occlusion"]
    else:
        current = random_map(w, h, dminl, size_d, seed)
    passes = []
    for _ in range(iterations):
        H = histogram(img_l, img_r, current, mark)
        T = table(H)
        r = dict(solve(cost(T, img_l, img_r, size_d, dminl), cost(T, img_l, img_r, size_d, dminr, right=True)))
        r["hist"], r["table"] = H, T
        passes.append(r)
        current = r["occlusion"]
    return passes


# ---- the scene of the feasibility check: one fixed relation between the gray values, not the identity ---------------------------
SCENE_W, SCENE_H, SCENE_D, SCENE_DMIN = 192, 48, 16, -15
SCENE_BG, SCENE_FG, SCENE_BAND = -4, -10, (70, 130)
SCENE_KEPT = ((16, 60), (70, 124), (136, 192))


def mapping(name):
    """A 256-entry look-up table for the right image."""
    v = np.arange(256, dtype=np.int64)
    if name == "invert":
        return (255 - v).astype(np.uint8)
    if name == "permute":
        return np.random.default_rng(20081).permutation(256).astype(np.uint8)
    if name == "fold":
        return np.abs(2 * v - 255).astype(np.uint8)
    raise ValueError(name)


def scene(seed, mapname, smooth=0):
    """-> (left, right, truth, kept): white noise (smoothed `smooth` times by a 5-point mean), the background at label -4, a band
    of label -10 in the left columns 70 .. 129, the right image sent through mapping(mapname); kept marks the 7392 pixels away
    from the image border and from the band's occlusions."""
    w, h, pad = SCENE_W, SCENE_H, 16
    tex = np.random.default_rng(seed).integers(0, 256, (h, w + pad)).astype(np.float64)
    for _ in range(smooth):
        p = np.pad(tex, 1, mode="edge")
        tex = (p[1:-1, 1:-1] + p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) / 5.0
    tex = np.rint(tex).astype(np.uint8)
    truth = np.full((h, w), SCENE_BG, np.int64)
    truth[:, SCENE_BAND[0]:SCENE_BAND[1]] = SCENE_FG
    x = np.arange(w)[None, :]
    left = np.take_along_axis(tex, x + truth + pad, axis=1)
    right = mapping(mapname)[tex[:, pad:]]
    kept = np.zeros((h, w), bool)
    for a, b in SCENE_KEPT:
        kept[:, a:b] = True
    return np.ascontiguousarray(left), np.ascontiguousarray(right), truth.astype(F32), kept


def wrong(disp, truth, kept):
    return int(np.count_nonzero((np.asarray(disp, F32) != truth) & kept))
