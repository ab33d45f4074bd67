"""numpy reference of PatchMatch stereo (smx_dev_patchmatch_pair / smx_dev_pm_plane_cost): the contract above smx_pm_params in
include/smx.h, float32 throughout, every operation rounded on its own in the stated order.

A view's state is four (h, w) float32 arrays: the plane (a, b, d0) and its cost m.  `plane_cost` evaluates planes at a list
of pixels (vectorised over the pixels and over the columns of one window row; the sum itself runs tap by tap, row-major, in
one accumulator).  `patchmatch` is the search; `slanted_scene` builds the demonstration scene of the tests.
"""
import numpy as np

F = np.float32
U32 = np.uint32
# spatial candidates (dx, dy) of a pixel, in the contract's order
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-5, 0), (5, 0), (0, -5), (0, 5))
DRAWS_PER_ITERATION = 32          # refinement steps a draw index leaves room for


class PMParams:
    def __init__(self, radius=8, gamma=10.0, iterations=4, max_slope=2.0, seed=0):
        self.radius, self.gamma, self.iterations, self.max_slope, self.seed = radius, gamma, iterations, max_slope, seed


def fmix32(h):
    """The 32-bit finaliser of MurmurHash3 (Appleby), on uint32 arrays."""
    h = np.asarray(h, U32).copy()
    with np.errstate(over="ignore"):
        h ^= h >> U32(16)
        h *= U32(0x85EBCA6B)
        h ^= h >> U32(13)
        h *= U32(0xC2B2AE35)
        h ^= h >> U32(16)
    return h


def pm_hash(seed, view, pix, draw):
    with np.errstate(over="ignore"):
        h = fmix32(np.asarray(seed, U32) + U32(0x9E3779B9) * (np.asarray(view, U32) + U32(1)))
        h = fmix32(h ^ np.asarray(pix, U32))
        return fmix32(h ^ np.asarray(draw, U32))


def uniform(seed, view, pix, draw):
    """U in [0, 1): (float)(hash >> 8) * 2^-24."""
    return (pm_hash(seed, view, pix, draw) >> U32(8)).astype(F) * F(2.0 ** -24)


def weights(gamma):
    return np.exp(-np.arange(256, dtype=np.float64) / float(gamma)).astype(F)


def cost_const(alpha, th_color, th_grad):
    """make_cost_const (smx_common.h) in numpy."""
    al = F(alpha)
    oma = F(1.0) - al
    tc, tg = F(th_color), F(th_grad)
    return {"alpha": al, "oma": oma, "th_color": tc, "th_grad": tg, "border": F(F(oma * tc) + F(al * tg))}


def xgrad(img):
    """The x derivative of the cost volume (oracle.xderiv); a one-column image has gradient 0."""
    I = np.asarray(img, np.uint8).astype(np.int32)
    h, w = I.shape
    g = np.zeros((h, w), np.int32)
    if w >= 2:
        g[:, 1:-1] = I[:, :-2] - I[:, 2:]
        g[:, 0] = I[:, 0] - I[:, 1]
        g[:, -1] = I[:, -2] - I[:, -1]
    return (g.astype(F) / F(2)).astype(F)


class View:
    """What one view's plane cost reads: its own gray image and gradient, the other view's, its label range."""

    def __init__(self, own, other, dmin, size_d, pm, cc):
        self.I = np.ascontiguousarray(own, np.uint8)
        self.h, self.w = self.I.shape
        self.If = self.I.astype(F)
        self.G = xgrad(own)
        self.O = np.asarray(other, np.uint8).astype(F)
        self.GO = xgrad(other)
        self.dmin, self.dmax = F(dmin), F(dmin + size_d - 1)
        self.size_d = size_d
        self.r = pm.radius
        self.tab = weights(pm.gamma)
        self.cc = cc


def plane_cost(v, ys, xs, a, b, d0):
    """m(p, f) for pixels (ys[k], xs[k]) and planes (a[k], b[k], d0[k]) -> float32 [len(ys)]."""
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    a, b, d0 = (np.asarray(t, F) for t in (a, b, d0))
    w, h, r, cc = v.w, v.h, v.r, v.cc
    acc = np.zeros(ys.shape, F)
    Ip = v.I[ys, xs].astype(np.int32)
    dxs = np.arange(-r, r + 1)
    fdx = dxs.astype(F)
    qx = xs[:, None] + dxs[None, :]
    okx = (qx >= 0) & (qx < w)
    qxc = np.clip(qx, 0, w - 1)
    fqx = qx.astype(F)
    wm1 = F(w - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        adx = (a[:, None] * fdx[None, :]).astype(F)
        base = (d0[:, None] + adx).astype(F)
        for dy in range(-r, r + 1):
            qy = ys + dy
            oky = (qy >= 0) & (qy < h)
            if not oky.any():
                continue
            row = np.clip(qy, 0, h - 1)[:, None]
            wgt = v.tab[np.abs(Ip[:, None] - v.I[row, qxc].astype(np.int32))]
            d = (base + (b * F(dy)).astype(F)[:, None]).astype(F)
            xf = (fqx + d).astype(F)
            inside = (d >= v.dmin) & (d <= v.dmax) & (xf >= F(0)) & (xf <= wm1)
            xsafe = np.where(inside, xf, F(0)).astype(F)
            fl = np.floor(xsafe)
            i = fl.astype(np.int64)
            t = (xsafe - fl).astype(F)
            i1 = np.minimum(i + 1, w - 1)
            o0, g0 = v.O[row, i], v.GO[row, i]
            Ii = (o0 + (t * (v.O[row, i1] - o0)).astype(F)).astype(F)
            Gi = (g0 + (t * (v.GO[row, i1] - g0)).astype(F)).astype(F)
            t1 = np.abs(v.If[row, qxc] - Ii)
            t2 = np.abs(v.G[row, qxc] - Gi)
            m1 = np.where(t1 < cc["th_color"], t1, cc["th_color"]).astype(F)
            m2 = np.where(t2 < cc["th_grad"], t2, cc["th_grad"]).astype(F)
            rho = ((cc["oma"] * m1).astype(F) + (cc["alpha"] * m2).astype(F)).astype(F)
            rho = np.where(inside, rho, cc["border"]).astype(F)
            term = (wgt * rho).astype(F)
            ok = oky[:, None] & okx
            for k in range(2 * r + 1):
                acc = np.where(ok[:, k], (acc + term[:, k]).astype(F), acc)
    return acc


def plane_cost_map(own, other, dmin, size_d, pm, cc, planes):
    """The cost of a whole plane map [3][h][w] of one view (smx_pm_plane_cost) -> [h][w]."""
    v = View(own, other, dmin, size_d, pm, cc)
    ys, xs = np.mgrid[0:v.h, 0:v.w]
    p = np.asarray(planes, F)
    return plane_cost(v, ys.ravel(), xs.ravel(), p[0].ravel(), p[1].ravel(), p[2].ravel()).reshape(v.h, v.w)


def _clamp(x, lo, hi):
    """By comparisons: a value equal to a bound stays itself, so the sign of a zero is defined."""
    x = np.asarray(x, F)
    return np.where(x < lo, F(lo), np.where(x > hi, F(hi), x)).astype(F)


def recentre(a_n, b_n, d0_n, x, y, nx, ny):
    """The disparity at (x, y) of the plane that pixel (nx, ny) holds."""
    return ((d0_n + (a_n * (x - nx).astype(F)).astype(F)).astype(F) + (b_n * (y - ny).astype(F)).astype(F)).astype(F)


def refinement_steps(size_d):
    """Delta_d of every refinement step: (size_d - 1) / 2 halved while it is at least 0.1."""
    out, dd = [], F(size_d - 1) * F(0.5)
    while dd >= F(0.1):
        out.append(dd)
        dd = F(dd * F(0.5))
    return out


class _State:
    def __init__(self, v, view, pm):
        self.v, self.view = v, view
        h, w = v.h, v.w
        ys, xs = np.mgrid[0:h, 0:w]
        self.ys, self.xs = ys.ravel(), xs.ravel()
        pix = (self.ys * w + self.xs).astype(U32)
        ms = F(pm.max_slope)
        u = [uniform(pm.seed, view, pix, k) for k in range(3)]
        self.d0 = (v.dmin + (u[0] * F(v.size_d - 1)).astype(F)).astype(F)
        self.a = (((F(2) * u[1]).astype(F) - F(1)).astype(F) * ms).astype(F)
        self.b = (((F(2) * u[2]).astype(F) - F(1)).astype(F) * ms).astype(F)
        self.m = plane_cost(v, self.ys, self.xs, self.a, self.b, self.d0)


def _pass(s, pm, it, colour):
    """Spatial propagation and refinement of the pixels of one colour of one view."""
    v = s.v
    h, w = v.h, v.w
    sel = np.nonzero(((s.xs + s.ys) & 1) == colour)[0]
    if sel.size == 0:
        return
    x, y = s.xs[sel], s.ys[sel]
    A, B, D, M = (t.reshape(h, w) for t in (s.a, s.b, s.d0, s.m))
    a, b, d0, m = s.a[sel].copy(), s.b[sel].copy(), s.d0[sel].copy(), s.m[sel].copy()
    cands = []
    for ddx, ddy in NEIGHBOURS:
        nx, ny = x + ddx, y + ddy
        ok = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
        nxc, nyc = np.clip(nx, 0, w - 1), np.clip(ny, 0, h - 1)
        an, bn = A[nyc, nxc], B[nyc, nxc]
        dn = recentre(an, bn, D[nyc, nxc], x, y, nxc, nyc)
        ok &= (dn >= v.dmin) & (dn <= v.dmax)
        c = np.full(sel.shape, np.inf, F)
        k = np.nonzero(ok)[0]
        if k.size:
            c[k] = plane_cost(v, y[k], x[k], an[k], bn[k], dn[k])
        cands.append((ok, an, bn, dn, c))
    for ok, an, bn, dn, c in cands:
        take = ok & (c < m)
        a, b, d0, m = np.where(take, an, a), np.where(take, bn, b), np.where(take, dn, d0), np.where(take, c, m)
    ms = F(pm.max_slope)
    ds = F(ms * F(0.5))
    pix = (y * w + x).astype(U32)
    for k, dd in enumerate(refinement_steps(v.size_d)):
        base = 3 + 3 * (it * DRAWS_PER_ITERATION + k)
        r = [((F(2) * uniform(pm.seed, s.view, pix, base + j)).astype(F) - F(1)).astype(F) for j in range(3)]
        dn = _clamp((d0 + (r[0] * dd).astype(F)).astype(F), v.dmin, v.dmax)
        an = _clamp((a + (r[1] * ds).astype(F)).astype(F), -ms, ms)
        bn = _clamp((b + (r[2] * ds).astype(F)).astype(F), -ms, ms)
        c = plane_cost(v, y, x, an, bn, dn)
        take = c < m
        a, b, d0, m = np.where(take, an, a), np.where(take, bn, b), np.where(take, dn, d0), np.where(take, c, m)
        ds = F(ds * F(0.5))
    s.a[sel], s.b[sel], s.d0[sel], s.m[sel] = a, b, d0, m


def _view_propagation(s, snap_other):
    v = s.v
    h, w = v.h, v.w
    ao, bo, do = (t.reshape(h, w) for t in snap_other)
    xo = np.floor(((s.xs.astype(F) + s.d0).astype(F) + F(0.5)).astype(F)).astype(np.int64)
    xo = np.clip(xo, 0, w - 1)
    an, bn, dn = -ao[s.ys, xo], -bo[s.ys, xo], -do[s.ys, xo]
    ok = (dn >= v.dmin) & (dn <= v.dmax)
    c = np.full(s.m.shape, np.inf, F)
    k = np.nonzero(ok)[0]
    if k.size:
        c[k] = plane_cost(v, s.ys[k], s.xs[k], an[k], bn[k], dn[k])
    take = ok & (c < s.m)
    s.a, s.b, s.d0, s.m = (np.where(take, n, o).astype(F) for n, o in ((an, s.a), (bn, s.b), (dn, s.d0), (c, s.m)))


def patchmatch(left, right, size_d, dminl, dminr, pm, cc):
    """-> dict: planes [2][3][h][w], cost, disp, label [2][h][w] (view 0 the left), all float32."""
    vl = View(left, right, dminl, size_d, pm, cc)
    vr = View(right, left, dminr, size_d, pm, cc)
    st = [_State(vl, 0, pm), _State(vr, 1, pm)]
    for it in range(pm.iterations):
        for s in st:
            _pass(s, pm, it, it & 1)
            _pass(s, pm, it, (it & 1) ^ 1)
        snaps = [(s.a.copy(), s.b.copy(), s.d0.copy()) for s in st]
        _view_propagation(st[0], snaps[1])
        _view_propagation(st[1], snaps[0])
    h, w = vl.h, vl.w
    planes = np.stack([np.stack([s.a, s.b, s.d0]).reshape(3, h, w) for s in st]).astype(F)
    cost = np.stack([s.m.reshape(h, w) for s in st]).astype(F)
    disp = planes[:, 2].copy()
    label = np.stack([_clamp(np.floor((s.d0 + F(0.5)).astype(F)), s.v.dmin, s.v.dmax).reshape(h, w) for s in st])
    return {"planes": planes, "cost": cost, "disp": disp, "label": label.astype(F)}


# ---- the demonstration scene: a slanted, textured surface -----------------------------------------------------------
SCENE_W, SCENE_H, SCENE_D, SCENE_DMINL, SCENE_X0 = 96, 32, 16, -15, 16


def slanted_scene(seed):
    """-> (left, right, truth): right is a box-blurred uniform-noise texture, left is warped from it with linear
    interpolation by the true left disparity -1.5 - 0.08 x - 0.10 y.  Compare on the columns >= SCENE_X0."""
    rng = np.random.default_rng(seed)
    w, h = SCENE_W, SCENE_H
    noise = rng.uniform(0.0, 255.0, (h + 2, w + 2))
    tex = sum(noise[i:i + h, j:j + w] for i in range(3) for j in range(3)) / 9.0
    # stretch the blurred texture back over the u8 range
    tex = np.clip((tex - 127.5) * 2.5 + 127.5, 0.0, 255.0)
    ys, xs = np.mgrid[0:h, 0:w]
    truth = -1.5 - 0.08 * xs - 0.10 * ys
    xm = np.clip(xs + truth, 0.0, w - 1.0)
    i0 = np.floor(xm).astype(np.int64)
    i1 = np.minimum(i0 + 1, w - 1)
    t = xm - i0
    left = tex[ys, i0] * (1.0 - t) + tex[ys, i1] * t
    return np.rint(left).astype(np.uint8), np.rint(tex).astype(np.uint8), truth.astype(np.float64)


def error_counts(disp, truth, x0=SCENE_X0):
    """(pixels off by more than 0.5, pixels off by more than 1) on the columns >= x0."""
    e = np.abs(np.asarray(disp, np.float64)[:, x0:] - truth[:, x0:])
    return int((e > 0.5).sum()), int((e > 1.0).sum())
