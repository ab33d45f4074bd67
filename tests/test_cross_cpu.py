"""The numpy reference of the cross-based aggregation (tests/cross_ref.py) on its own: against a scalar brute force that walks
every arm pixel by pixel and sums pixel by pixel over the region, its bounds and fixed points, a case worked by hand, and the
scene the feature exists for.  Then the refusals of the C-ABI entries and of the Python layers, none of which needs a GPU: an
invalid argument is SMX_E_ARG (-1) before any device call (a device call on a machine without a GPU would be SMX_E_HIP, -2).
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cross_ref as ref

H, W, D = 24, 64, 8


def textured_guide(h=H, w=W, seed=3, channels=3):
    """Blocks of 8 x 8 in nearby colours with +-3 noise: arms of every length, cut by either threshold"""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(90, 120, ((h + 7) // 8, (w + 7) // 8, channels))
    g = np.kron(blocks, np.ones((8, 8, 1), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w, channels))
    return g.astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# scalar brute force
# ---------------------------------------------------------------------------------------------
def brute_arms(guide, l1, l2, tau1, tau2):
    I = guide.astype(np.int64).tolist()
    h, w = len(I), len(I[0])
    dist = lambda a, b: max(abs(x - y) for x, y in zip(a, b))
    out = np.zeros((4, h, w), np.int32)
    for y in range(h):
        for x in range(w):
            p = I[y][x]
            for e, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
                k, prev = 0, p
                for j in range(1, l1 + 1):
                    qy, qx = y + j * dy, x + j * dx
                    if not (0 <= qy < h and 0 <= qx < w):
                        break
                    q = I[qy][qx]
                    if not (dist(q, p) < tau1 and dist(q, prev) < tau1 and (j <= l2 or dist(q, p) < tau2)):
                        break
                    k, prev = j, q
                out[e, y, x] = k
    return out


def brute_region_sum(V, a, order):
    """V (D, h, w) int64; every region pixel by pixel (all slices of a pixel at once)"""
    _, h, w = V.shape
    S = np.zeros_like(V)
    l, r, u, d = (a[k].tolist() for k in range(4))
    for y in range(h):
        for x in range(w):
            acc = np.zeros(V.shape[0], np.int64)
            if order == 0:
                for yy in range(y - u[y][x], y + d[y][x] + 1):
                    for xx in range(x - l[yy][x], x + r[yy][x] + 1):
                        acc += V[:, yy, xx]
            else:
                for xx in range(x - l[y][x], x + r[y][x] + 1):
                    for yy in range(y - u[y][xx], y + d[y][xx] + 1):
                        acc += V[:, yy, xx]
            S[:, y, x] = acc
    return S


@pytest.fixture(scope="module")
def textured():
    g = textured_guide()
    par = dict(l1=9, l2=4, tau1=20, tau2=6)
    a = ref.arms(g, **par)
    cost = (np.random.default_rng(5).random((D, H, W)) * 300 - 20).astype(np.float32)
    return g, par, a, cost


def test_arms_against_the_brute_force(textured):
    g, par, a, _ = textured
    assert np.array_equal(a, brute_arms(g, **par))
    assert len(np.unique(a)) == par["l1"] + 1                  # every arm length occurs
    for ch in (1, 4):
        g2 = textured_guide(channels=ch, seed=4)
        assert np.array_equal(ref.arms(g2, 17, 17, 12, 5), brute_arms(g2[:, :, :3], 17, 17, 12, 5))
    # a gray guide as (h, w) and as (h, w, 1); a fourth byte is ignored
    g1 = textured_guide(channels=1)
    assert np.array_equal(ref.arms(g1[:, :, 0], **par), ref.arms(g1, **par))
    g4 = np.concatenate((g, np.random.default_rng(0).integers(0, 256, (H, W, 1), dtype=np.uint8)), axis=2)
    assert np.array_equal(ref.arms(g4, **par), a)
    packed = ref.pack_arms(a)
    assert packed.dtype == np.uint32 and np.array_equal((packed >> 16) & 255, a[2])


@pytest.mark.parametrize("order", [0, 1])
def test_one_iteration_against_the_brute_force(textured, order):
    g, par, a, cost = textured
    V = 16 * ref.clamp_cost(cost)
    S = brute_region_sum(V, a, order)
    assert np.array_equal(ref.region_sum(V, a, order), S)
    area = brute_region_sum(np.ones((1, H, W), np.int64), a, order)[0]
    assert np.array_equal(ref.areas(a)[order], area)
    assert np.array_equal(ref.iterate(V, a, ref.areas(a), order), (2 * S + area) // (2 * area))
    if order == 0:
        assert np.array_equal(ref.aggregate_int(g, cost, iterations=1, **par), (2 * S + area) // (2 * area))


def test_the_two_orders_differ(textured):
    _, _, a, _ = textured
    ar = ref.areas(a)
    assert np.any(ar[0] != ar[1])


def test_clamp():
    c = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 0.99, 1.0, 254.99, 255.0, 255.5, 1e30, np.inf], np.float32)
    assert ref.clamp_cost(c).tolist() == [0, 0, 0, 0, 0, 0, 1, 254, 255, 255, 255, 255]


@pytest.mark.parametrize("l1", [1, 17, 63])
def test_bounds(l1):
    rng = np.random.default_rng(l1)
    g = textured_guide(40, 150, seed=l1)
    cost = rng.choice(np.array([0, 255, 300, 128.5, -3], np.float32), (3, 40, 150))
    for par in (dict(l1=l1, l2=l1 // 2, tau1=20, tau2=6), dict(l1=l1, l2=0, tau1=256, tau2=256)):
        a = ref.arms(g, **par)
        ar = ref.areas(a)
        assert ar.min() >= 1 and ar.max() <= (2 * l1 + 1) ** 2
        assert a.min() >= 0 and a.max() <= l1
        for it in (1, 4):
            V = ref.aggregate_int(g, cost, iterations=it, **par)
            assert V.min() >= 0 and V.max() <= 4080
    S = ref.region_sum(np.full((1, 40, 150), 4080, np.int64), a, 0)
    assert S.max() < 1 << 26


def test_a_constant_volume_stays_constant():
    g = textured_guide()
    for c in (0.0, 1.0, 77.0, 255.0, 1000.0):
        cost = np.full((2, H, W), c, np.float32)
        for it in (1, 2, 3, 4):
            q = ref.aggregate(g, cost, l1=17, l2=8, tau1=20, tau2=6, iterations=it)
            assert (q == min(c, 255.0)).all()


def test_open_thresholds_give_the_clamped_box():
    rng = np.random.default_rng(11)
    g = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    cost = rng.integers(0, 256, (D, H, W)).astype(np.float32)
    l1 = 5
    a = ref.arms(g, l1=l1, l2=0, tau1=256, tau2=256)
    yy, xx = np.mgrid[0:H, 0:W]
    assert np.array_equal(a, np.minimum(l1, np.stack((xx, W - 1 - xx, yy, H - 1 - yy))))
    V = 16 * cost.astype(np.int64)
    want = np.empty_like(V)
    for y in range(H):
        for x in range(W):
            box = V[:, max(0, y - l1):y + l1 + 1, max(0, x - l1):x + l1 + 1]
            area = box.shape[1] * box.shape[2]
            want[:, y, x] = (2 * box.sum(axis=(1, 2)) + area) // (2 * area)
    assert np.array_equal(ref.aggregate_int(g, cost, l1=l1, l2=0, tau1=256, tau2=256, iterations=1), want)
    # both orders sum the same box
    assert np.array_equal(ref.region_sum(V, a, 0), ref.region_sum(V, a, 1))


def test_a_case_worked_by_hand():
    """3 x 3, l1 = l2 = 1: the 50s are an edge.  Arms, the areas of the horizontal-first order and one iteration, by hand."""
    g = np.array([[10, 10, 50], [10, 10, 50], [10, 10, 10]], np.uint8)
    cost = np.arange(1, 10, dtype=np.float32).reshape(1, 3, 3)
    a = ref.arms(g, l1=1, l2=1, tau1=20, tau2=6)
    assert a[0].tolist() == [[0, 1, 0], [0, 1, 0], [0, 1, 1]]          # left
    assert a[1].tolist() == [[1, 0, 0], [1, 0, 0], [1, 1, 0]]          # right
    assert a[2].tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 0]]          # up
    assert a[3].tolist() == [[1, 1, 1], [1, 1, 0], [0, 0, 0]]          # down
    assert ref.pack_arms(a)[1, 1] == 1 | 0 << 8 | 1 << 16 | 1 << 24
    assert ref.areas(a)[0].tolist() == [[4, 4, 2], [6, 7, 2], [4, 5, 2]]
    # H = [[3, 3, 3], [9, 9, 6], [15, 24, 17]] in units of the cost; S = [[12, 12, 9], [27, 36, 9], [24, 33, 17]]
    V = ref.aggregate_int(g, cost, l1=1, l2=1, tau1=20, tau2=6, iterations=1)
    assert V[0].tolist() == [[48, 48, 72], [72, 82, 72], [96, 106, 136]]
    q = ref.aggregate(g, cost, l1=1, l2=1, tau1=20, tau2=6, iterations=1)
    assert q.dtype == np.float32 and q[0].tolist() == [[3.0, 3.0, 4.5], [4.5, 5.125, 4.5], [6.0, 6.625, 8.5]]


def test_the_tie_rule():
    q = np.zeros((4, 2, 2), np.float32)
    assert (ref.winners(q) == 3).all()


# ---------------------------------------------------------------------------------------------
# the reason for the feature
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_the_step_between_two_colours_of_equal_luminance(iterations):
    """Two textureless surfaces, (150, 60, 60) and (60, 105, 60) with +-2 noise, true labels 2 and 5, random costs 20 .. 59 with
    the true slice drawn from 10 .. 49.  With the colour thresholds every winner is right; with the same arm length and the
    thresholds opened to a plain box, pixels along the step are wrong."""
    g, cost, truth = ref.step_scene(seed=1)
    assert g.shape == (24, 64, 3) and cost.shape == (8, 24, 64)
    q = ref.aggregate(g, cost, l1=17, l2=8, tau1=20, tau2=6, iterations=iterations)
    assert np.array_equal(ref.winners(q), truth)
    box = ref.aggregate(g, cost, l1=17, l2=8, tau1=256, tau2=256, iterations=iterations)
    wrong = ref.winners(box) != truth
    assert wrong.any() and wrong[:, 32 - 17:32 + 17].sum() == wrong.sum()


# ---------------------------------------------------------------------------------------------
# refusals: no GPU needed
# ---------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(l1=0), dict(l1=64), dict(l2=-1), dict(l2=35), dict(tau2=0), dict(tau1=5), dict(tau1=257, tau2=257),
              dict(tau1=257), dict(iterations=0), dict(iterations=5), dict(l1=-3, l2=-3)]


def _params(**kw):
    p = smx.default_cross_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_and_workspace_size():
    L = smx.lib()
    p = smx.default_cross_params()
    assert (p.l1, p.l2, p.tau1, p.tau2, p.iterations) == (34, 17, 20, 6, 4)
    assert ref.params_ok(**ref.DEFAULTS) and ref.DEFAULTS == {k: getattr(p, k) for k in ref.DEFAULTS}
    n = 7 * 5
    assert L.smx_cross_workspace_bytes(7, 5, 1, 1) == 255 + 20 * n and L.smx_cross_workspace_bytes(7, 5, 1, 2) == 255 + 40 * n
    assert L.smx_cross_workspace_bytes(7, 5, 3, 2) == 255 + 2 * (8 + 36) * n
    assert L.smx_cross_workspace_bytes(1, 70000, 1, 1) > 0              # (no bound on h alone)
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 1, 3), (65536, 32768, 1, 1)):
        assert L.smx_cross_workspace_bytes(*bad) == 0, bad


def test_every_entry_refuses_invalid_arguments_before_any_device_call():
    L = smx.lib()
    x = C.c_void_p(4096)            # never dereferenced: every call below fails its checks
    wsb = L.smx_cross_workspace_bytes(7, 5, 2, 2)

    def arms(p, gl=x, gr=x, ch=3, w=7, h=5, out=x):
        return L.smx_dev_cross_arms(p, gl, gr, ch, w, h, out, None)

    def pair(p, gl=x, gr=x, ch=3, cl=x, cr=x, w=7, h=5, s0=0, s1=2, keys=x, ws=x, wsb=wsb):
        return L.smx_dev_cross_wta_pair(p, gl, gr, ch, cl, cr, w, h, s0, s1, keys, None, None, None, ws, wsb, None)

    def host(p, g=x, ch=3, cost=x, best=x, dmap=x, w=7, h=5, D=2):
        return L.smx_cross_aggregate(p, g, ch, cost, best, dmap, None, w, h, D, 0)

    for bad in BAD_PARAMS:
        assert not ref.params_ok(**{**ref.DEFAULTS, **bad}), bad
        p = C.byref(_params(**bad))
        for entry in (arms, pair, host):
            assert entry(p) == -1, (entry.__name__, bad)
            assert b"l1" in L.smx_last_error()
    ok = C.byref(_params())
    for entry in (arms, pair, host):
        assert entry(None) == -1
        for kw in (dict(ch=2), dict(ch=0), dict(ch=5), dict(w=0), dict(h=0), dict(w=65536, h=32768)):
            assert entry(ok, **kw) == -1, (entry.__name__, kw)
    for kw in (dict(gl=None, gr=None), dict(out=None)):
        assert arms(ok, **kw) == -1, kw
    for kw in (dict(cl=None, cr=None, gl=None, gr=None), dict(gl=None), dict(cr=None), dict(keys=None), dict(s0=-1), dict(s0=2),
               dict(s0=3, s1=2)):
        assert pair(ok, **kw) == -1, kw
    for kw in (dict(g=None), dict(cost=None), dict(best=None), dict(dmap=None), dict(D=0)):
        assert host(ok, **kw) == -1, kw
    # the workspace: too small for one slice, or missing, is SMX_E_WS before anything is launched
    assert pair(ok, wsb=L.smx_cross_workspace_bytes(7, 5, 1, 2) - 1) == -3 and b"workspace" in L.smx_last_error()
    assert pair(ok, ws=None) == -3
    assert pair(ok, gr=None, cr=None, wsb=L.smx_cross_workspace_bytes(7, 5, 1, 1) - 1) == -3
    assert L.smx_ctx_set_cross(None, ok) == -1


def test_the_python_layers_refuse():
    from stereo_matching_cuda_amd.device import PairPipeline
    cost = np.zeros((2, 5, 7), np.float32)
    best, dmap = smx.init_wta(5, 7)
    with pytest.raises(ValueError):
        smx.cross_aggregate(np.zeros((5, 7, 2), np.uint8), cost, best, dmap, 0)
    with pytest.raises(ValueError):
        smx.cross_aggregate(np.zeros((5, 7, 3), np.uint8), cost[:, :4], best, dmap, 0)
    with pytest.raises(ValueError):
        smx.cross_aggregate(np.zeros((5, 7), np.uint8), cost, best.astype(np.float64), dmap, 0)
    with pytest.raises(smx.SmxError) as e:
        smx.cross_aggregate(np.zeros((5, 7), np.uint8), cost, best, dmap, 0, params=_params(l1=64))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        PairPipeline(64, 24, 8, aggregation="cross", guidance="rgb", device="cpu")
    with pytest.raises(ValueError):
        PairPipeline(64, 24, 8, aggregation="bogus", device="cpu")
    assert isinstance(smx.default_cross_params(), _lib.CrossParams) and smx.CrossParams is _lib.CrossParams
