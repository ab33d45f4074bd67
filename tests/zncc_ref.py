"""numpy reference of the ZNCC window matching cost, written from the definition of include/smx.h (smx_zncc_params), not from
the kernels: a loop over the window's taps, int64 sums, and the float32 steps one at a time.  It is not a box filter, so it
shares no running sum with the kernel.

  moments(I)[y][x]: S = sum of I_ext over the (2 rx + 1) x (2 ry + 1) window, Q = sum of I_ext^2, V = N Q - S^2
              (replicate clamp: I_ext[y][x] = I[clamp(y)][clamp(x)]).  The device word is S | V << 32.
  cost[z][y][x], d = dmin + z, xx = x + d:  255 if xx is outside 0 .. w-1; else with
              P = sum over the window of A_ext[y+dy][x+dx] * B_ext[y+dy][xx+dx], num = N P - S_A(y, x) S_B(y, xx):
              128 if V_A(y, x) == 0 or V_B(y, xx) == 0, else
              nf = f32(|num|), s = min((nf * nf) / (f32(Va) * f32(Vb)), 1), c = 127.5 (1 - s) or 127.5 (1 + s) for num < 0,
              cost = rint(c) -- every step in float32.
"""
import numpy as np

DEFAULTS = (3, 3)            # rx, ry
OUTSIDE, FLAT = np.float32(255.0), np.float32(128.0)


def window(rx, ry):
    return (2 * rx + 1) * (2 * ry + 1)


def _ext(img, dy, dx, xs=None):
    """img_ext[y + dy][xs + dx] for every y and the columns xs (default: every x), replicate-clamped, as int64."""
    h, w = img.shape
    xs = np.arange(w) if xs is None else xs
    return img[np.clip(np.arange(h) + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)].astype(np.int64)


def moments(img, rx=3, ry=3):
    """(S, V) of every pixel, int64 (h, w) each."""
    img = np.asarray(img, np.uint8)
    S = np.zeros(img.shape, np.int64)
    Q = np.zeros(img.shape, np.int64)
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            v = _ext(img, dy, dx)
            S += v
            Q += v * v
    return S, window(rx, ry) * Q - S * S


def moment_words(img, rx=3, ry=3):
    """The device's 8-byte word of every pixel: S | V << 32, uint64 (h, w)."""
    S, V = moments(img, rx, ry)
    return S.astype(np.uint64) | (V.astype(np.uint64) << np.uint64(32))


def zncc_cost(i1, i2, size_d, dmin, rx=3, ry=3, s_begin=0, s_end=None, stats=None):
    """Slices [s_begin, s_end) of the volume of i1 (the view's own image) against i2.  stats: a dict that receives the largest
    |num|, N P, S_A S_B and V met, for the overflow bounds."""
    A, B = np.asarray(i1, np.uint8), np.asarray(i2, np.uint8)
    h, w = A.shape
    s_end = size_d if s_end is None else s_end
    N = window(rx, ry)
    Sa, Va = moments(A, rx, ry)
    Sb, Vb = moments(B, rx, ry)
    if stats is not None:
        stats["V"] = max(stats.get("V", 0), int(Va.max()), int(Vb.max()))
    cost = np.full((s_end - s_begin, h, w), OUTSIDE, np.float32)
    f32 = np.float32
    for z in range(s_begin, s_end):
        d = dmin + z
        x0, x1 = max(0, -d), min(w, w - d)           # the x with 0 <= x + d < w
        if x0 >= x1:
            continue
        xs = np.arange(x0, x1)
        P = np.zeros((h, x1 - x0), np.int64)
        for dy in range(-ry, ry + 1):
            for dx in range(-rx, rx + 1):
                P += _ext(A, dy, dx, xs) * _ext(B, dy, dx, xs + d)
        sa, sb = Sa[:, x0:x1], Sb[:, x0 + d:x1 + d]
        va, vb = Va[:, x0:x1], Vb[:, x0 + d:x1 + d]
        num = N * P - sa * sb
        if stats is not None:
            for k, v in (("num", np.abs(num).max()), ("NP", (N * P).max()), ("SS", (sa * sb).max())):
                stats[k] = max(stats.get(k, 0), int(v))
        flat = (va == 0) | (vb == 0)
        nf = np.abs(num).astype(f32)
        den = va.astype(f32) * vb.astype(f32)
        den = np.where(flat, f32(1.0), den)
        s = np.minimum((nf * nf) / den, f32(1.0))
        c = np.where(num >= 0, f32(127.5) * (f32(1.0) - s), f32(127.5) * (f32(1.0) + s)).astype(f32)
        cost[z - s_begin, :, x0:x1] = np.where(flat, FLAT, np.rint(c)).astype(f32)
    return cost


# ---- the scene of the feasibility check: a gain and an offset that change across the image ----------------------------------
SCENE_W, SCENE_H, SCENE_D, SCENE_DMIN = 192, 48, 16, -15
SCENE_BG, SCENE_FG, SCENE_COLS = -4, -10, (70, 130)          # the labels, and the left image's columns of the foreground
SCENE_TREND, SCENE_NOISE = (150.0, 50.0), 20                 # the texture: a brightness trend across the width + white noise
SCENE_GAIN, SCENE_OFFSET = (0.6, 1.4), (0.0, 80.0)           # of the right image, at its left and its right edge
SCENE_BAND = (14, 34)                                        # the rows of the periodic pattern
SCENE_PERIOD, SCENE_STEP, SCENE_WRAP, SCENE_CONTRAST = 7, 6, 16, (2, 5)
# away from the image border, from the occlusions beside the foreground and from the foreground's own first columns, where a
# window of radius 3 still straddles the depth edge (every window cost fattens an edge by its radius; not what this scene asks)
SCENE_KEPT = ((16, 60), (74, 124), (136, 192))


def scene(seed):
    """-> (left, right, truth, kept).  The world is a wide texture: a brightness trend from 150 down to 50 across the width plus
    white noise of +-20.  In the rows SCENE_BAND it holds a pattern of period 7 along x, constant along y: every period repeats
    one ORDER of values with a contrast of its own (2 .. 5, drawn per period) and lies 6 above the one before, all of it above
    all of the one before (the steps start again every 16 periods).  Background at label -4, the left columns 70 .. 129 at
    label -10.  The right image is the world times a gain ramp 0.6 .. 1.4 plus an offset ramp 0 .. 80 across its width,
    rounded and clipped to u8: the right image grows brighter where the left one grows darker, while every window keeps
    right = a left + b with a > 0."""
    w, h, pad = SCENE_W, SCENE_H, 16
    rng = np.random.default_rng(seed)
    xw = np.arange(w + pad)
    trend = SCENE_TREND[0] + (SCENE_TREND[1] - SCENE_TREND[0]) * xw / (w + pad - 1.0)
    tex = trend[None, :] + rng.integers(-SCENE_NOISE, SCENE_NOISE + 1, (h, w + pad))
    P = SCENE_PERIOD
    order = rng.permutation(P) / (P - 1.0)                                   # one order of P values in 0 .. 1
    k = xw // P
    contrast = rng.integers(SCENE_CONTRAST[0], SCENE_CONTRAST[1] + 1, k.max() + 1)
    tex[SCENE_BAND[0]:SCENE_BAND[1]] = (20 + SCENE_STEP * (k % SCENE_WRAP) + contrast[k] * order[xw % P])[None, :]
    tex = np.rint(tex)
    truth = np.full((h, w), SCENE_BG, np.int64)
    truth[:, SCENE_COLS[0]:SCENE_COLS[1]] = SCENE_FG
    left = np.take_along_axis(tex, np.arange(w)[None, :] + truth + pad, axis=1)
    t = np.arange(w) / (w - 1.0)
    gain = SCENE_GAIN[0] + (SCENE_GAIN[1] - SCENE_GAIN[0]) * t
    offset = SCENE_OFFSET[0] + (SCENE_OFFSET[1] - SCENE_OFFSET[0]) * t
    right = np.clip(np.rint(tex[:, pad:] * gain[None, :] + offset[None, :]), 0, 255)
    kept = np.zeros((h, w), bool)
    for a, b in SCENE_KEPT:
        kept[:, a:b] = True
    return (np.ascontiguousarray(left.astype(np.uint8)), np.ascontiguousarray(right.astype(np.uint8)), truth.astype(np.float32),
            kept)


def wrong(disp, truth, kept):
    return int(np.count_nonzero((np.asarray(disp, np.float32) != truth) & kept))
