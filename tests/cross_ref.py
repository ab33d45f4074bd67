"""numpy reference of the cross-based aggregation as include/smx.h defines it (smx_dev_cross_arms, smx_dev_cross_wta_pair):
integers throughout, the arms by plain loops over the arm length, the sums by integer cumsum.  A plain helper module, imported
by name: tests/test_cross_cpu.py holds it against a scalar brute force that sums pixel by pixel over the region;
tests/test_gpu_cross.py holds the kernels against it, bit for bit.
"""
import numpy as np

F32 = np.float32
DEFAULTS = dict(l1=34, l2=17, tau1=20, tau2=6, iterations=4)


def params_ok(l1, l2, tau1, tau2, iterations):
    return 1 <= l1 <= 63 and 0 <= l2 <= l1 and 1 <= tau2 <= tau1 <= 256 and 1 <= iterations <= 4


def _channels(guide):
    """(h, w, 1 or 3) int32: the bytes the colour distance reads (a fourth byte is ignored)"""
    g = np.asarray(guide)
    assert g.dtype == np.uint8 and g.ndim in (2, 3)
    if g.ndim == 2:
        g = g[:, :, None]
    assert g.shape[2] in (1, 3, 4)
    return g[:, :, :3].astype(np.int32)


def arms(guide, l1=34, l2=17, tau1=20, tau2=6):
    """(4, h, w) int32: the arms left, right, up, down of every pixel"""
    I = _channels(guide)
    h, w = I.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((4, h, w), np.int32)
    for e, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
        alive = np.ones((h, w), bool)
        for j in range(1, l1 + 1):
            qy, qx = yy + j * dy, xx + j * dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            cy, cx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            py, px = np.clip(qy - dy, 0, h - 1), np.clip(qx - dx, 0, w - 1)          # q_{j-1}
            d_p = np.abs(I[cy, cx] - I).max(axis=2)
            d_prev = np.abs(I[cy, cx] - I[py, px]).max(axis=2)
            ok = inside & (d_p < tau1) & (d_prev < tau1)
            if j > l2:
                ok &= d_p < tau2
            alive &= ok
            if not alive.any():
                break
            out[e] += alive
    return out


def pack_arms(a):
    """(h, w) uint32: l | r << 8 | u << 16 | d << 24"""
    a = a.astype(np.uint32)
    return a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24)


def clamp_cost(cost):
    """SGM's clamp of a float32 cost to an integer 0 .. 255; NaN gives 0"""
    c = np.asarray(cost, F32)
    with np.errstate(invalid="ignore"):
        inner = np.where(c <= 255, np.trunc(np.where(np.isfinite(c), c, 0)), 255)
        return np.where(c >= 0, inner, 0).astype(np.int64)


def _hsum(V, a):
    """sum of V[..., y, x'] over x - l <= x' <= x + r"""
    h, w = V.shape[-2:]
    P = np.zeros(V.shape[:-1] + (w + 1,), np.int64)
    np.cumsum(V, axis=-1, out=P[..., 1:])
    x = np.arange(w)[None, :]
    hi = np.broadcast_to(x + a[1] + 1, V.shape)
    lo = np.broadcast_to(x - a[0], V.shape)
    return np.take_along_axis(P, hi, axis=-1) - np.take_along_axis(P, lo, axis=-1)


def _vsum(V, a):
    """sum of V[..., y', x] over y - u <= y' <= y + d"""
    h, w = V.shape[-2:]
    P = np.zeros(V.shape[:-2] + (h + 1, w), np.int64)
    np.cumsum(V, axis=-2, out=P[..., 1:, :])
    y = np.arange(h)[:, None]
    hi = np.broadcast_to(y + a[3] + 1, V.shape)
    lo = np.broadcast_to(y - a[2], V.shape)
    return np.take_along_axis(P, hi, axis=-2) - np.take_along_axis(P, lo, axis=-2)


def region_sum(V, a, order):
    """order 0: horizontal first (HV), order 1: vertical first (VH)"""
    return _vsum(_hsum(V, a), a) if order == 0 else _hsum(_vsum(V, a), a)


def areas(a):
    """(2, h, w) int64: area_HV, area_VH"""
    one = np.ones(a.shape[1:], np.int64)
    return np.stack((region_sum(one, a, 0), region_sum(one, a, 1)))


def iterate(V, a, ar, i):
    """V_{i+1} from V_i: iteration i counts from 0"""
    S = region_sum(V, a, i & 1)
    return (2 * S + ar[i & 1]) // (2 * ar[i & 1])


def aggregate_int(guide, cost, l1=34, l2=17, tau1=20, tau2=6, iterations=4):
    """V_iterations [z][y][x] int64 (four fractional bits) of a cost volume [z][y][x]"""
    assert params_ok(l1, l2, tau1, tau2, iterations)
    a = arms(guide, l1, l2, tau1, tau2)
    ar = areas(a)
    V = 16 * clamp_cost(cost)
    for i in range(iterations):
        V = iterate(V, a, ar, i)
    return V


def aggregate(guide, cost, **kw):
    """q [z][y][x] f32"""
    return (aggregate_int(guide, cost, **kw).astype(F32) * F32(0.0625)).astype(F32)


def winners(q):
    """(h, w) slice index of the winner: the last slice of equal costs wins"""
    D = q.shape[0]
    return D - 1 - np.argmin(q[::-1], axis=0)


def step_scene(seed=7, h=24, w=64, D=8, split=32):
    """Two textureless surfaces of equal luminance and different colour with a disparity step between them, and noisy costs:
    (guide (h, w, 3) uint8, cost (D, h, w) float32, truth (h, w) labels)."""
    rng = np.random.default_rng(seed)
    guide = np.empty((h, w, 3), np.int32)
    guide[:, :split] = (150, 60, 60)
    guide[:, split:] = (60, 105, 60)
    guide = (guide + rng.integers(-2, 3, guide.shape)).astype(np.uint8)
    truth = np.where(np.arange(w)[None, :] < split, 2, 5) * np.ones((h, 1), np.int64)
    cost = rng.integers(20, 60, (D, h, w)).astype(F32)
    np.put_along_axis(cost, truth[None], rng.integers(10, 50, (1, h, w)).astype(F32), axis=0)
    return guide, cost, truth
