"""The scan-line optimiser with colour-adaptive penalties without a GPU: the numpy reference (tests/scanline_ref.py) against a
scalar brute force written here from the definition in include/smx.h, the properties that follow from the definition, the
scene that shows what the adaptive penalties are for, and the argument checks of the library's entry points."""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cross_ref
import scanline_ref as ref
import sgm_ref

DIRS8 = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]


def _dist(g, ax, ay, bx, by):
    a, b = g[ay][ax], g[by][bx]
    if np.ndim(a) == 0:
        return abs(int(a) - int(b))
    return max(abs(int(a[c]) - int(b[c])) for c in range(min(3, len(a))))


def brute_force(guide_own, guide_other, cost, dmin, p1, p2, tau_so, paths):
    """S by the definition, one scalar at a time; every path walked from its own start pixel."""
    D, h, w = cost.shape
    Cv = [[[0] * w for _ in range(h)] for _ in range(D)]
    for d in range(D):
        for y in range(h):
            for x in range(w):
                c = float(cost[d, y, x])
                Cv[d][y][x] = (int(c) if c <= 255 else 255) if c >= 0 else 0
    P = [(p1, p2), (p1 // 4, p2 // 4), (p1 // 10, p2 // 10)]
    S = np.zeros((D, h, w), np.int64)
    for dx, dy in DIRS8[:paths]:
        for y0 in range(h):
            for x0 in range(w):
                if 0 <= y0 - dy < h and 0 <= x0 - dx < w:
                    continue                                   # not the start of a path
                x, y, prev = x0, y0, None
                while 0 <= x < w and 0 <= y < h:
                    cur = []
                    for z in range(D):
                        if prev is None:
                            cur.append(Cv[z][y][x])
                            continue
                        e1 = _dist(guide_own, x, y, x - dx, y - dy) >= tau_so
                        qx = x + dmin + z
                        e2 = False
                        if 0 <= qx < w and 0 <= qx - dx < w and 0 <= y - dy < h:
                            e2 = _dist(guide_other, qx, y, qx - dx, y - dy) >= tau_so
                        P1, P2 = P[int(e1) + int(e2)]
                        m = min(prev)
                        t = [prev[z], m + P2]
                        if z - 1 >= 0:
                            t.append(prev[z - 1] + P1)
                        if z + 1 < D:
                            t.append(prev[z + 1] + P1)
                        cur.append(Cv[z][y][x] + min(t) - m)
                    for z in range(D):
                        S[z, y, x] += cur[z]
                    prev = cur
                    x, y = x + dx, y + dy
    return S


def _volume(seed, D, h, w, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (D, h, w)).astype(np.float32)


def _guide(seed, h, w, ch=3):
    g = (100 + np.random.default_rng(seed).integers(0, 26, (h, w, ch))).astype(np.uint8)
    return g[:, :, 0].copy() if ch == 1 else g


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("w,h,D,dmin", [(1, 1, 1, 0), (1, 6, 3, 0), (6, 1, 2, -1), (5, 9, 4, -3), (9, 7, 5, -2), (3, 11, 5, 1),
                                        (7, 4, 3, 7), (7, 4, 3, -10), (4, 6, 6, -4)])
@pytest.mark.parametrize("seed", [0, 1])
def test_reference_against_brute_force(paths, w, h, D, dmin, seed):
    """(5, 9), (3, 11), (4, 6): w < h, the diagonals of the kernels' column walk wrap; dmin 7 / -10: every partner outside."""
    cost = _volume(seed, D, h, w, 256 if seed else 63)
    ch = (1, 3, 4)[(w + h + seed) % 3]
    go, gx = _guide(seed + 10, h, w, ch), _guide(seed + 20, h, w, ch)
    for p1, p2, tau in ((127, 382, 15), (0, 0, 15), (3, 39, 12), (3, 4095, 1), (10, 120, 256)):
        got = ref.aggregate(go, gx, cost, dmin, p1, p2, tau, paths)
        assert np.array_equal(got, brute_force(go, gx, cost, dmin, p1, p2, tau, paths)), (p1, p2, tau)


@pytest.mark.parametrize("paths", [4, 8])
def test_tau_256_equals_sgm_bit_for_bit(paths):
    cost = _volume(3, 9, 8, 13)
    go, gx = _guide(1, 8, 13), _guide(2, 8, 13)
    for p1, p2 in ((10, 120), (0, 0), (4095, 4095)):
        a = ref.outputs(go, gx, cost, -4, p1=p1, p2=p2, tau_so=256, paths=paths)
        b = sgm_ref.outputs(cost, p1, p2, paths)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_the_comparison_with_tau_is_greater_or_equal():
    g = np.full((1, 6), 50, np.uint8)
    g[0, 2:] = 65           # a step of exactly 15
    g[0, 4:] = 79           # a step of 14
    e = ref.edges(g, 1, 0, 15)
    assert e[0].tolist() == [False, False, True, False, False, False]
    assert ref.edges(g, 1, 0, 14)[0].tolist() == [False, False, True, False, True, False]
    assert ref.edges(g, -1, 0, 15)[0].tolist() == [False, True, False, False, False, False]      # p - r is the right neighbour
    assert not ref.edges(g, 1, 0, 256).any()


def test_e1_alone_e2_alone_and_both():
    """One row, one label, dmin = 2: the partner of x is x + 2."""
    flat = np.full((1, 8), 50, np.uint8)
    own = flat.copy(); own[0, 3:] = 90             # own edge at x = 3
    other = flat.copy(); other[0, 5:] = 90         # the other view's edge at column 5, the partner of x = 3
    k = lambda a, b: ref.edge_count(a, b, 1, 0, 2, 1, 15)[0, 0].tolist()
    assert k(own, flat) == [0, 0, 0, 1, 0, 0, 0, 0]
    assert k(flat, other) == [0, 0, 0, 1, 0, 0, 0, 0]
    assert k(own, other) == [0, 0, 0, 2, 0, 0, 0, 0]
    other2 = flat.copy(); other2[0, 6:] = 90
    assert k(own, other2) == [0, 0, 0, 1, 1, 0, 0, 0]
    # and the penalties they select, in floor division
    cost = np.zeros((2, 1, 8), np.float32); cost[1] = 200
    for a, b, div in ((flat, flat, 1), (own, flat, 4), (flat, other, 4), (own, other, 10)):
        k2 = np.stack([ref.edge_count(a, b, 1, 0, 2, 1, 15)[0]] * 2)          # the same flags for both labels
        L = ref.path_costs(ref.clamp(cost), k2, 1, 0, 30, 99)
        assert L[1, 0, 3] == 200 + 30 // div, div


def test_a_partner_outside_the_image_and_a_partner_whose_predecessor_is_outside():
    g = np.full((3, 5), 50, np.uint8)
    g[:, 0] = 200                                # every step out of column 0 is an edge in the other view
    flat = np.full((3, 5), 50, np.uint8)
    # direction (1, 0), dmin -1: the partner of x is x - 1; x = 0 has none, x = 1 has column 0 whose predecessor is outside,
    # x = 2 has column 1, whose step from column 0 is an edge
    k = ref.edge_count(flat, g, 1, 0, -1, 1, 15)[0]
    assert k[1].tolist() == [0, 0, 1, 0, 0]
    # direction (-1, 0): the predecessor is the right neighbour: partner 0 (of x = 1) sees the step 200 -> 50
    assert ref.edge_count(flat, g, -1, 0, -1, 1, 15)[0, 1].tolist() == [0, 1, 0, 0, 0]
    # the last column's partner lies outside on the right with dmin = +1
    g2 = flat.copy(); g2[:, 4] = 200
    assert ref.edge_count(flat, g2, 1, 0, 1, 1, 15)[0, 1].tolist() == [0, 0, 0, 1, 0]
    assert ref.edge_count(flat, g2, -1, 0, 1, 1, 15)[0, 1].tolist() == [0, 0, 1, 0, 0]
    # a vertical direction: the partner's predecessor lies in the row above; row 0 has none
    g3 = flat.copy(); g3[1:, :] = 200
    assert ref.edge_count(flat, g3, 0, 1, 0, 1, 15)[0].tolist() == [[0] * 5, [1] * 5, [0] * 5]
    # every partner outside: k is e1 alone
    for dmin in (5, -5, 1 << 20, -(1 << 20)):
        assert np.array_equal(ref.edge_count(g, g3, 1, 0, dmin, 3, 15), np.broadcast_to(ref.edges(g, 1, 0, 15), (3, 3, 5)))


def test_the_fourth_channel_is_ignored_and_one_channel_is_gray():
    rng = np.random.default_rng(4)
    g3 = (100 + rng.integers(0, 26, (6, 9, 3))).astype(np.uint8)
    g4 = np.concatenate((g3, rng.integers(0, 256, (6, 9, 1)).astype(np.uint8)), axis=2)
    cost = _volume(5, 4, 6, 9)
    assert np.array_equal(ref.aggregate(g3, g3[::-1].copy(), cost, -1), ref.aggregate(g4, g4[::-1].copy(), cost, -1))
    gray = g3[:, :, 0].copy()
    assert np.array_equal(ref.aggregate(gray, gray, cost), ref.aggregate(gray[:, :, None], gray[:, :, None], cost))
    assert np.array_equal(ref.aggregate(gray, gray, cost), ref.aggregate(np.repeat(gray[:, :, None], 3, 2), np.repeat(gray[:, :, None], 3, 2), cost))


def test_small_penalties_floor_to_zero():
    """p1 < 4 gives P1 = 0 on an edge: with p2 < 4 as well, an edge in front of every pixel removes every penalty."""
    h, w, D = 5, 7, 4
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (100 + 40 * ((yy + xx) & 1)).astype(np.uint8)           # every horizontal and vertical step is an edge
    cost = _volume(6, D, h, w)
    S = ref.aggregate(checker, checker, cost, 1 << 20, p1=3, p2=3, tau_so=15, paths=4)      # no partner: k = 1
    assert np.array_equal(S, 4 * ref.clamp(cost))
    assert not np.array_equal(ref.aggregate(checker, checker, cost, 1 << 20, p1=4, p2=4, tau_so=15, paths=4), 4 * ref.clamp(cost))
    # k = 2 wherever the partner and its predecessor are inside: 39 // 10 = 3, 39 // 4 = 9
    k = ref.edge_count(checker, checker, 1, 0, 0, 1, 15)[0]
    assert (k[:, 1:] == 2).all() and (k[:, 0] == 0).all()


# ---- the scene -------------------------------------------------------------------------------------------------------
def _wrong(z, truth):
    strip = np.zeros(truth.shape, bool)
    strip[:, 30:33] = True
    bad = z != truth
    return int((bad & strip).sum()), int((bad & ~strip).sum())


def test_thin_scene():
    """A strip three pixels wide in front of a weakly textured surface (72 strip pixels, 1 464 of the background; paths 4,
    tau_so 15; the counts are wrong winners on the strip + on the background).  No constant pair of penalties gets the scene
    right: small ones leave the surface noisy, large ones erase the strip.  The adaptive rule at 40 / 400 gets every pixel."""
    gl, gr, cost, truth = ref.thin_scene()
    assert _wrong(sgm_ref.winners(sgm_ref.clamp(cost)), truth) == (29, 698)
    want = {(4, 40): ((16, 305), (10, 305)), (10, 120): ((15, 135), (5, 136)), (20, 200): ((16, 11), (2, 16)),
            (40, 400): ((26, 0), (0, 0))}
    for (p1, p2), (const, adaptive) in want.items():
        c = _wrong(sgm_ref.outputs(cost, p1, p2, 4)["z"], truth)
        a = _wrong(ref.outputs(gl, gr, cost, 0, p1=p1, p2=p2, tau_so=15, paths=4)["z"], truth)
        print(f"p {p1}, {p2}: constant {c[0]} + {c[1]}, adaptive {a[0]} + {a[1]}")
        assert c == const and a == adaptive, (p1, p2, c, a)
        assert sum(c) >= 10
    assert want[(40, 400)][1] == (0, 0)


def test_thin_scene_behind_the_cross_aggregation():
    """The chain cross -> scan line: the aggregated volume's own winners are all correct; constant penalties at 40 / 400
    destroy 18 strip pixels of it, adaptive ones none."""
    gl, gr, cost, truth = ref.thin_scene()
    q = cross_ref.aggregate(gl, cost, l1=17, l2=8, tau1=20, tau2=6, iterations=2)
    assert _wrong(cross_ref.winners(q), truth) == (0, 0)
    c = _wrong(sgm_ref.outputs(q, 40, 400, 4)["z"], truth)
    a = _wrong(ref.outputs(gl, gr, q, 0, p1=40, p2=400, tau_so=15, paths=4)["z"], truth)
    print(f"chain: constant {c[0]} + {c[1]}, adaptive {a[0]} + {a[1]}")
    assert c == (18, 0) and a == (0, 0)
    assert sum(a) == 0 and sum(c) > 0


# ---- host-only C ABI -------------------------------------------------------------------------------------------------
def _p(p1=127, p2=382, tau_so=15, paths=4):
    p = _lib.ScanlineParams()
    p.p1, p.p2, p.tau_so, p.paths = p1, p2, tau_so, paths
    return p


def test_defaults():
    p = smx.default_scanline_params()
    assert (p.p1, p.p2, p.tau_so, p.paths) == (127, 382, 15, 4)
    assert isinstance(p, smx.ScanlineParams)
    assert ref.DEFAULTS == dict(p1=127, p2=382, tau_so=15, paths=4)


BAD = [dict(p1=11, p2=10), dict(p2=4096), dict(p1=-1), dict(paths=5), dict(paths=0), dict(tau_so=0), dict(tau_so=257),
       dict(tau_so=-3), dict(size_d=257), dict(size_d=0), dict(channels=2), dict(channels=0), dict(channels=5), dict(w=0),
       dict(h=0), dict(w=65536, h=32768)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_are_refused_by_every_entry_without_a_gpu(bad):
    L = smx.lib()
    buf = np.zeros(4 * 4 * 8, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    kw = dict(p1=127, p2=382, tau_so=15, paths=4, size_d=4, channels=3, w=4, h=4)
    kw.update(bad)
    p = _p(kw["p1"], kw["p2"], kw["tau_so"], kw["paths"])
    assert not ref.params_ok(p.p1, p.p2, p.tau_so, p.paths) or set(bad) & {"size_d", "channels", "w", "h"}
    w, h, D, ch = kw["w"], kw["h"], kw["size_d"], kw["channels"]
    assert L.smx_dev_scanline_wta_pair(C.byref(p), ptr, ptr, ch, ptr, ptr, w, h, D, 0, 0, ptr, None, None, None, ptr, 1 << 40,
                                       None) == -1
    assert L.smx_last_error()
    assert L.smx_scanline_optimize(C.byref(p), ptr, ptr, ch, ptr, None, ptr, ptr, w, h, D, 0) == -1
    if set(bad) & {"size_d", "w", "h"}:
        assert L.smx_scanline_workspace_bytes(w, h, D, 2) == 0


def test_null_pointers_and_a_short_workspace_are_refused_without_a_gpu():
    L = smx.lib()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p()
    tail = (4, 4, 4, -3, 0, ptr, None, None, None)
    call = L.smx_dev_scanline_wta_pair
    assert call(None, ptr, ptr, 3, ptr, ptr, *tail, ptr, 1 << 40, None) == -1
    assert call(C.byref(p), ptr, ptr, 3, None, None, *tail, ptr, 1 << 40, None) == -1
    assert call(C.byref(p), None, ptr, 3, ptr, ptr, *tail, ptr, 1 << 40, None) == -1          # both guides always
    assert call(C.byref(p), ptr, None, 3, ptr, None, *tail, ptr, 1 << 40, None) == -1
    assert call(C.byref(p), ptr, ptr, 3, ptr, ptr, 4, 4, 4, 0, 0, None, None, None, None, ptr, 1 << 40, None) == -1
    for l, r, nviews in ((ptr, ptr, 2), (ptr, None, 1), (None, ptr, 1)):
        need = L.smx_scanline_workspace_bytes(4, 4, 4, nviews)
        assert call(C.byref(p), ptr, ptr, 3, l, r, *tail, ptr, need - 1, None) == -3
        assert call(C.byref(p), ptr, ptr, 3, l, r, *tail, None, need, None) == -3
    assert L.smx_scanline_optimize(C.byref(p), None, ptr, 3, ptr, None, ptr, ptr, 4, 4, 4, 0) == -1
    assert L.smx_scanline_optimize(C.byref(p), ptr, None, 3, ptr, None, ptr, ptr, 4, 4, 4, 0) == -1
    assert L.smx_scanline_optimize(C.byref(p), ptr, ptr, 3, None, None, ptr, ptr, 4, 4, 4, 0) == -1
    with pytest.raises(ValueError):
        smx.scanline_optimize(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError):
        smx.scanline_optimize(np.zeros((4, 5), np.uint8), np.zeros((4, 5), np.uint8), np.zeros((2, 4, 4), np.float32))


def test_workspace_bytes():
    ws, sgm = smx.lib().smx_scanline_workspace_bytes, smx.lib().smx_sgm_workspace_bytes
    assert ws(0, 5, 4, 1) == 0 and ws(5, 0, 4, 1) == 0 and ws(5, 5, 0, 1) == 0 and ws(5, 5, 257, 1) == 0
    assert ws(5, 5, 4, 0) == 0 and ws(5, 5, 4, 3) == 0 and ws(65536, 32768, 4, 1) == 0
    # the SGM workspace plus one byte per pixel and view of edge flags, 8 bytes of padding a row, each plane rounded to 256
    for w, h, d in ((7, 5, 9), (64, 64, 64), (129, 70, 70), (1242, 375, 192), (1, 1, 1)):
        for v in (1, 2):
            extra = ws(w, h, d, v) - sgm(w, h, d, v)
            assert 2 * h * (w + 8) <= extra <= 2 * (h * (w + 8) + 255), (w, h, d, v)
