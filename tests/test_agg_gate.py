"""Which aggregation runs for which smx_params, checked on the CPU.

Every entry point asks one host function (agg_path_for, exported as the test hook smx_debug_agg_path) whether the call runs
the multi-kernel path (1), the ring walker (2), FAST (4) or the comb walker (5).  Each fused walker is bit-exact only inside
its own argument; outside it the multi-kernel path, which evaluates the reference's arithmetic
literally, must run.  Here the argument is restated in Python and the hook is checked against it on every boundary value,
on each side of it, and on seeded random parameter sets; then the one part of the argument that depends on the thresholds
-- the sentinel cell of a partner outside the image saturating the truncation -- is emulated in numpy for every parameter
set the hook sends to a walker.  No GPU: the hook is host arithmetic.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

INT_MAX, INT_MIN = 2**31 - 1, -2**31
SENTINEL = 60000.0                        # k_v4_guid_rows: both halves of a cell outside the image
PIXELS = np.arange(256, dtype=np.float32)                       # pixel values
DERIVS = (np.arange(-255, 256, dtype=np.float32) / 2).astype(np.float32)   # x-derivatives: -127.5, -127, ..., 127.5
RING_TH_COLOR_MAX = 59745                 # |255 - 60000| in f32
RING_TH_GRAD_MAX = 59872                  # floor(|127.5 - 60000|) in f32 (thresholds are integers)
COMB_TH_COLOR_MAX = 59744                 # RN16(60000 - 255)
COMB_TH_GRAD_MAX = 59872                  # RN16(60000 - 127.5)


@pytest.fixture(scope="module")
def so():
    if not os.path.exists(_lib.SO_PATH):
        smx.build()
    _lib.lib()
    L = C.CDLL(_lib.SO_PATH)
    L.smx_debug_agg_path.restype = C.c_int
    L.smx_debug_agg_path.argtypes = [C.POINTER(_lib.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_int)]
    L.smx_debug_v5_fix_bytes.restype = C.c_int
    L.smx_debug_v5_fix_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    L.smx_last_error.restype = C.c_char_p
    return L


def hook(so, p, w, h, nviews, use_cost, forced):
    """(path, None) or (None, error message)."""
    out = C.c_int(-1)
    rc = so.smx_debug_agg_path(C.byref(p), w, h, nviews, int(use_cost), forced, C.byref(out))
    if rc == 0:
        return out.value, None
    assert rc == -1, rc                                       # SMX_E_ARG
    return None, so.smx_last_error().decode()


def fix_bytes(so, w, h, nviews):
    b = C.c_uint64()
    assert so.smx_debug_v5_fix_bytes(w, h, nviews, C.byref(b)) == 0
    return b.value


def params(**kw):
    p = smx.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- the gates, restated ------------------------------------------------------------------------------------------
def _f32(x):
    with np.errstate(over="ignore"):
        return np.float32(x)


def _fp16_exact(t):
    with np.errstate(over="ignore"):
        return float(np.float16(t)) == float(t)


def ring_applies(p, use_cost):
    """radius 0 .. 9; costs built from the images also need the sentinel to saturate both truncations in f32."""
    if not 0 <= p.radius <= 9:
        return False
    return use_cost or (p.th_color <= RING_TH_COLOR_MAX and p.th_grad <= RING_TH_GRAD_MAX)


def comb_applies(p, w, h, nviews, use_cost, fix):
    """radius 9, eps in [1, 1e30) compared in double, the planes within one 2 GiB descriptor;
    materialised costs: at least one 16-byte quad per plane (the values are checked on the device); costs built from the
    images: alpha and the thresholds after their f32 conversion in [0, 1] / [0, 1e6), the smallest nonzero term of each
    truncation >= 2^-60, thresholds exact in fp16 and at or below the nearest a cell comes to the sentinel in fp16."""
    if p.radius != 9 or not (p.eps >= 1.0 and p.eps < 1e30) or fix >= 2**31:
        return False
    if use_cost:
        return w * h >= 4
    a = _f32(p.alpha)
    oma = np.float32(1) - a
    thc, thg = _f32(p.th_color), _f32(p.th_grad)
    if not (0 <= a <= 1 and 0 <= thc < 1e6 and 0 <= thg < 1e6):
        return False
    t1 = oma * min(thc, np.float32(1))                       # |dI| >= 1 (integers)
    t2 = a * min(thg, np.float32(0.5))                       # |dg| >= 0.5 (halves)
    if not all(t == 0 or t >= 2.0**-60 for t in (t1, t2)):
        return False
    return (_fp16_exact(thc) and _fp16_exact(thg) and thc <= COMB_TH_COLOR_MAX and thg <= COMB_TH_GRAD_MAX)


def expected(p, w, h, nviews, use_cost, forced, fix):
    """(path, reason word of the error or None)."""
    if forced == 1:
        return 1, None
    if not ring_applies(p, use_cost):
        if forced == 0:
            return 1, None
        return None, "radius" if p.radius > 9 else "th_color"
    comb = comb_applies(p, w, h, nviews, use_cost, fix)
    if forced == 5 and not comb:
        return None, "comb walker"
    if forced == 3:
        return 2, None
    if forced == 4:
        return 4, None
    return (5 if comb else 2), None


# ---- boundary values ----------------------------------------------------------------------------------------------
def _f32_below(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


def _f32_above(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


RADII = [0, 1, 8, 9, 10, 12]
EPS = [math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 6.5025, 1e29, math.nextafter(1e30, 0.0), 1e30,
       math.nextafter(1e30, math.inf), math.inf, math.nan, 0.5, 0.0, -1.0]
ALPHAS = [0.0, -0.0, -1e-50, -1e-30, 2.0**-59, _f32_below(2.0**-59), 2.0**-59 * (1 - 2.0**-40), 2.0**-60, 0.3, 1 / 3, 0.9,
          _f32_below(1.0), 1.0, 1 + 1e-12, _f32_above(1.0), 1.5, -0.5, math.nan]
TH_COLOR = [INT_MIN, -1, 0, 1, 7, 255, 256, 2047, 2048, 2049, 2050, 4096, 4097, 59743, 59744, 59745, 59746, 59776, 59968,
            59999, 60000, 65504, 65535, 65536, 999999, 1000000, INT_MAX]
TH_GRAD = [INT_MIN, -1, 0, 1, 2, 127, 128, 2049, 59840, 59871, 59872, 59873, 59904, 59936, 59968, 60000, 65504, 1000000,
           INT_MAX]


def _one_at_a_time():
    """Each parameter over its boundary values, the others at the defaults, at radius 8 and 9."""
    for radius in (8, 9):
        yield params(radius=radius)
        for e in EPS:
            yield params(radius=radius, eps=e)
        for a in ALPHAS:
            yield params(radius=radius, alpha=a)
        for t in TH_COLOR:
            yield params(radius=radius, th_color=t)
            yield params(radius=radius, th_color=t, alpha=0.0)
        for t in TH_GRAD:
            yield params(radius=radius, th_grad=t)
            yield params(radius=radius, th_grad=t, alpha=1.0)
    for r in RADII:
        yield params(radius=r)
    for tc in TH_COLOR:                                      # the two thresholds together
        for tg in (0, 2, 59872, 59873, 60000):
            yield params(th_color=tc, th_grad=tg)
    yield params(alpha=2.0**-59, th_color=0, eps=1e29)       # the denormal regime of the a_k


def _random(n, seed=2024):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        p = smx.default_params()
        p.radius = int(rng.choice([0, 3, 8, 9, 9, 9, 9, 10, 11]))
        p.eps = float(rng.choice(EPS)) if rng.random() < 0.5 else float(10.0 ** rng.uniform(-3, 31))
        p.alpha = float(rng.choice(ALPHAS)) if rng.random() < 0.5 else float(rng.uniform(-0.1, 1.1))
        p.th_color = int(rng.choice(TH_COLOR)) if rng.random() < 0.5 else int(rng.integers(-10, 70000))
        p.th_grad = int(rng.choice(TH_GRAD)) if rng.random() < 0.5 else int(rng.integers(-10, 70000))
        if rng.random() < 0.3:                               # fp16-exact thresholds near the sentinel
            p.th_color = int(32 * rng.integers(1860, 1880))
            p.th_grad = int(32 * rng.integers(1865, 1880))
        if rng.random() < 0.3:                               # inside the comb walker's domain but for the thresholds
            p.radius, p.eps, p.alpha = 9, float(10.0 ** rng.uniform(0, 29.9)), float(rng.uniform(0, 1))
        if rng.random() < 0.2:                               # fp16-exact thresholds anywhere below 65536
            e = int(rng.integers(0, 16))
            p.th_color = int(rng.integers(0, 1024) << e >> 4) if e >= 4 else int(rng.integers(0, 2049))
            p.th_grad = int(rng.choice([0, 1, 2, 127, 128, 2048, 59840, 59872, 59904]))
        yield p


def _fmt(p):
    return (f"radius={p.radius} eps={p.eps!r} alpha={p.alpha!r} th_color={p.th_color} th_grad={p.th_grad}")


def _check(so, p, w, h, nviews, use_cost, forced, fix):
    got, msg = hook(so, p, w, h, nviews, use_cost, forced)
    want, word = expected(p, w, h, nviews, use_cost, forced, fix)
    where = f"{_fmt(p)} {w}x{h} nviews={nviews} use_cost={use_cost} forced={forced}"
    assert got == want, f"{where}: hook {got} ({msg}), restatement {want}"
    if want is None:
        assert word in msg, f"{where}: the error should name the reason ({word}): {msg}"


def test_gate_on_every_boundary_value(so):
    w, h = 330, 25
    fix = {nv: fix_bytes(so, w, h, nv) for nv in (1, 2)}
    n = 0
    for p in _one_at_a_time():
        for nviews in (1, 2):
            for use_cost in (False, True):
                for forced in range(6):
                    _check(so, p, w, h, nviews, use_cost, forced, fix[nviews])
                    n += 1
    assert n > 5000


def test_gate_on_random_parameter_sets(so):
    rng = np.random.default_rng(7)
    shapes = [(2, 1), (3, 1), (2, 2), (330, 25), (1242, 375), (8192, 5460)]
    fix = {(w, h, nv): fix_bytes(so, w, h, nv) for (w, h) in shapes for nv in (1, 2)}
    for p in _random(2000):
        w, h = shapes[int(rng.integers(len(shapes)))]
        nviews, use_cost, forced = int(rng.integers(1, 3)), bool(rng.integers(2)), int(rng.integers(6))
        _check(so, p, w, h, nviews, use_cost, forced, fix[(w, h, nviews)])


def test_gate_at_the_descriptor_bound(so):
    """The comb walker only while its one-descriptor region stays below 2 GiB: the last image height inside and the
    first outside, for one view and for two."""
    w = 8192
    for nviews in (1, 2):
        lo, hi = 1, 20000                                    # fix(lo) < 2^31 <= fix(hi)
        assert fix_bytes(so, w, lo, nviews) < 2**31 <= fix_bytes(so, w, hi, nviews)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fix_bytes(so, w, mid, nviews) < 2**31 else (lo, mid)
        for h, comb in ((lo, True), (hi, False)):
            for use_cost in (False, True):
                assert hook(so, params(), w, h, nviews, use_cost, 0)[0] == (5 if comb else 2)
                for forced in range(6):
                    _check(so, params(), w, h, nviews, use_cost, forced, fix_bytes(so, w, h, nviews))


def test_workspace_size_follows_the_gate(so):
    """smx_agg_workspace_bytes_for sizes for the path the parameters run: a walker's workspace is smaller than the multi-kernel
    path needs, so parameters that leave the walkers must get the multi-kernel bound."""
    L = _lib.lib()
    w, h, n = 330, 25, 24
    multi = L.smx_agg_workspace_bytes(w, h, n)
    for p, fused in ((params(), True), (params(radius=3), True), (params(th_color=RING_TH_COLOR_MAX), True),
                     (params(radius=10), False), (params(th_color=RING_TH_COLOR_MAX + 1), False),
                     (params(th_grad=RING_TH_GRAD_MAX + 1), False), (params(radius=8, th_color=INT_MAX), False)):
        got = L.smx_agg_workspace_bytes_for(C.byref(p), w, h, n)
        assert (got < multi) if fused else (got == multi), _fmt(p)


# ---- the sentinel ----------------------------------------------------------------------------------------------------
def _oracle_border(orc, p):
    """costVolume.cu:184 as the oracle evaluates it: every partner of a 1 x 2 image at disparity 10 is outside."""
    img = np.zeros((1, 2), np.uint8)
    return orc.cost_volume(img, img, 1, 10, params=orc.Params.from_buffer_copy(bytes(p)))[0, 0, 0]


def _walker_border_costs(p, walker):
    """Every cost a walker forms against the sentinel cell, over all pixel values and derivatives of the own cell: the ring
    walker in f32 (cost_pair, smx_agg_dev.h), the comb walker in packed halves (cost_trunc_h2 + v_fma_mix_f32,
    smx_agg_v5.hip).  The weighted terms depend on one component each, so their distinct values are combined."""
    a = _f32(p.alpha)
    oma = np.float32(1) - a
    thc, thg = _f32(p.th_color), _f32(p.th_grad)
    if walker == 2:
        s = np.float32(SENTINEL)
        m1 = np.minimum(np.abs(PIXELS - s), thc)
        m2 = np.minimum(np.abs(DERIVS - s), thg)
    else:
        s = np.float16(SENTINEL)
        m1 = np.minimum(np.abs(PIXELS.astype(np.float16) - s), np.float16(thc)).astype(np.float32)
        m2 = np.minimum(np.abs(DERIVS.astype(np.float16) - s), np.float16(thg)).astype(np.float32)
    t1 = np.unique(oma * m1)
    t2 = np.unique(a * m2)
    return (t1[:, None] + t2[None, :]).ravel()


def _param_sets():
    yield from _one_at_a_time()
    yield from _random(2000)


def test_sentinel_saturates_wherever_a_walker_runs(so, orc):
    """For every parameter set the hook sends to a fused walker (costs built from the images), the cost of a partner outside
    the image must be the border constant of costVolume.cu:184 for every own cell: the sentinel must saturate both
    truncations.  (Thresholds just below 60000 pass the fp16 test but not this one.)"""
    checked = {2: 0, 5: 0}
    for p in _param_sets():
        for forced, walkers in ((0, None), (3, (2,))):
            path, _ = hook(so, p, 330, 25, 2, False, forced)
            if path not in (2, 5):
                continue
            border = np.float32(_oracle_border(orc, p)).view(np.uint32)
            for walker in walkers or (path,):
                got = _walker_border_costs(p, walker).view(np.uint32)
                bad = got != border
                assert not bad.any(), (f"{_fmt(p)} path {forced} -> walker {walker}: out-of-range cost "
                                       f"{got[bad][:3].view(np.float32)} != border {border.view(np.float32)}")
                checked[walker] += 1
    assert checked[2] > 1000 and checked[5] > 200, checked
