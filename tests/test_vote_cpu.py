"""The numpy reference of region voting and 16-direction interpolation (tests/vote_ref.py) on its own: against a scalar brute
force that walks every region pixel by pixel with a dict for its histogram, the two thresholds and the tie rule on maps built by
hand, the Jacobi rounds, every direction of the interpolation, and the scene the feature exists for.  Then the refusals of the
C-ABI entries and of the Python layers, none of which needs a GPU: an invalid argument is SMX_E_ARG (-1) before any device call
(a device call on a machine without a GPU would be SMX_E_HIP, -2).
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import cross_ref
import vote_ref as ref
from test_cross_cpu import textured_guide

F32 = np.float32
H, W, D = 24, 64, 8
INV = F32(-100)             # the LR check's marker with dmin = 0


def box_arms(h, w, l1):
    """the arms of a constant guide: l1 everywhere, cut at the border"""
    return cross_ref.arms(np.full((h, w), 7, np.uint8), l1=l1, l2=0, tau1=20, tau2=6)


# ---------------------------------------------------------------------------------------------
# scalar brute force
# ---------------------------------------------------------------------------------------------
def brute_round(disp, a, dmin, size_d, tau_s, tau_h_pct):
    d = disp.tolist()
    h, w = disp.shape
    l, r, u, dn = (a[k].tolist() for k in range(4))
    out = disp.copy()

    def label(v):
        if not np.isfinite(v):
            return None, False
        t = max(-2 ** 31, min(2 ** 31 - 1, int(v)))             # int() truncates toward zero
        valid = F32(min(t, 2 ** 31)) >= F32(dmin)
        return (t - dmin if valid and 0 <= t - dmin < size_d else None), bool(valid)

    for y in range(h):
        for x in range(w):
            if label(d[y][x])[1]:
                continue
            hist = {}
            for yy in range(y - u[y][x], y + dn[y][x] + 1):
                for xx in range(x - l[yy][x], x + r[yy][x] + 1):
                    b = label(d[yy][xx])[0]
                    if b is not None:
                        hist[b] = hist.get(b, 0) + 1
            total = sum(hist.values())
            if not hist:
                continue
            top = max(hist.values())
            b = max(k for k, c in hist.items() if c == top)
            if total > tau_s and 100 * top > tau_h_pct * total:
                out[y, x] = F32(dmin + b)
    return out


def noisy_map(rng, h, w, dmin, size_d, holes=0.3):
    d = (dmin + rng.integers(0, size_d, (h // 4 + 1, w // 8 + 1))).astype(F32)
    d = np.kron(d, np.ones((4, 8), F32))[:h, :w].copy()
    m = rng.random((h, w))
    d[m < holes] = dmin - 100
    d[(m > 0.95)] = dmin + size_d                       # valid, out of range
    d[(m > 0.93) & (m <= 0.95)] += F32(0.5)
    return d


@pytest.mark.parametrize("dmin, pct, tau_s", [(0, 40, 20), (-5, 0, 0), (-3, 60, 3)])
def test_voting_against_the_brute_force(dmin, pct, tau_s):
    rng = np.random.default_rng(17 + pct)
    g = textured_guide()
    a = cross_ref.arms(g, l1=9, l2=4, tau1=20, tau2=6)
    d = noisy_map(rng, H, W, dmin, D)
    rounds = []
    got = ref.vote(d, a, dmin, D, tau_s, pct, 3, rounds=rounds)
    want = d
    for k in range(3):
        want = brute_round(want, a, dmin, D, tau_s, pct)
        assert np.array_equal(rounds[k].view(np.uint32), want.view(np.uint32)), k
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (rounds[0] != d).any()
    # a valid pixel never changes, and the packed form of the arms gives the same
    v = ref.valid(d, dmin)
    assert np.array_equal(got[v].view(np.uint32), d[v].view(np.uint32))
    assert np.array_equal(ref.unpack_arms(cross_ref.pack_arms(a)), a)


def test_the_histograms_count_the_region():
    """with every pixel a voter S is area_HV"""
    g = textured_guide()
    a = cross_ref.arms(g, l1=9, l2=4, tau1=20, tau2=6)
    d = np.full((H, W), 3, F32)
    labels, hist = ref.histograms(d, a, 0, D)
    assert labels.tolist() == [3] and np.array_equal(hist[0], cross_ref.areas(a)[0])


# ---------------------------------------------------------------------------------------------
# thresholds, tie rule, Jacobi: maps built by hand on one row with box arms of 20 (the region of x = 20 is the whole row)
# ---------------------------------------------------------------------------------------------
def row_case(values):
    """a row of 41 pixels, the outlier in the middle, `values` spread over the other 40 (the rest invalid)"""
    d = np.full((1, 41), INV)
    others = [x for x in range(41) if x != 20]
    for x, v in zip(others, values):
        d[0, x] = v
    return d, box_arms(1, 41, 20)


def middle(d, a, **kw):
    return ref.vote(d, a, 0, D, iterations=1, **kw)[0, 20]


def test_tau_s_is_strict():
    d, a = row_case([3] * 20)
    assert middle(d, a, tau_s=20, tau_h_pct=40) == INV                  # S == tau_s
    assert middle(d, a, tau_s=19, tau_h_pct=40) == 3
    d, a = row_case([3] * 21)
    assert middle(d, a, tau_s=20, tau_h_pct=40) == 3                    # tau_s + 1


def test_tau_h_pct_is_strict():
    d, a = row_case([3] * 8 + [1] * 6 + [6] * 6)                        # S = 20, H = 8: 100 * 8 == 40 * 20
    assert middle(d, a, tau_s=5, tau_h_pct=40) == INV
    assert middle(d, a, tau_s=5, tau_h_pct=39) == 3
    d, a = row_case([3] * 9 + [1] * 6 + [6] * 6)                        # one vote more: 900 > 840
    assert middle(d, a, tau_s=5, tau_h_pct=40) == 3
    stats = {}
    ref.vote(*row_case([3] * 8 + [1] * 6 + [6] * 6), 0, D, 5, 40, 1, stats=stats)
    assert stats["reject_h"] >= 1


def test_a_tie_takes_the_larger_bin():
    d, a = row_case([2] * 10 + [5] * 10)
    assert middle(d, a, tau_s=5, tau_h_pct=40) == 5
    d, a = row_case([5] * 10 + [2] * 10)
    assert middle(d, a, tau_s=5, tau_h_pct=40) == 5
    d, a = row_case([2] * 10 + [5] * 10 + [7] * 10)
    assert middle(d, a, tau_s=5, tau_h_pct=20) == 7


def test_a_valid_pixel_outside_the_range_is_kept_and_not_counted():
    d, a = row_case([3] * 20 + [D] * 10 + [F32(D + 0.5)] * 5)          # 15 valid pixels with a bin behind the range
    out = ref.vote(d, a, 0, D, 20, 40, 1)
    assert out[0, 20] == INV                                             # S is 20, not 35
    assert np.array_equal(out.view(np.uint32), d.view(np.uint32))
    assert ref.valid(d, 0).sum() == 35 and ref.voters(d, 0, D)[0].sum() == 20
    # the bin is that of the truncated value: 3.75 votes for 3
    d, a = row_case([F32(3.75)] * 21)
    assert middle(d, a, tau_s=20, tau_h_pct=40) == 3


def test_the_rounds_are_jacobi():
    """Regions of 7 pixels on a row, S >= 3 needed: a round moves the front by one pixel; an in-place sweep by all of them."""
    d = np.full((1, 30), INV)
    d[0, :6] = 3
    a = box_arms(1, 30, 3)
    kw = dict(tau_s=2, tau_h_pct=40)
    one = ref.vote(d, a, 0, D, iterations=1, **kw)
    two = ref.vote(d, a, 0, D, iterations=2, **kw)
    assert (one[0] == 3).sum() == 7 and (two[0] == 3).sum() == 8          # the second round fills what the first could not
    assert two[0, 7] == 3 and one[0, 7] == INV
    sweep = d.copy()                                                     # the same rule in place, left to right
    for x in range(30):
        if sweep[0, x] == INV and (sweep[0, max(0, x - 3):x + 4] == 3).sum() > 2:
            sweep[0, x] = 3
    assert (sweep == 3).all() and not np.array_equal(sweep, one)
    eight = ref.vote(d, a, 0, D, iterations=8, **kw)
    assert (eight[0] == 3).sum() == 14


# ---------------------------------------------------------------------------------------------
# interpolation
# ---------------------------------------------------------------------------------------------
GUIDE9 = np.full((9, 9), 100, np.uint8)


def interp(d, guide=GUIDE9, disp_r=None, dmin=0, size_d=D, d_lr=0, stats=None):
    return ref.interpolate(d, guide, disp_r, dmin, size_d, d_lr, stats)


@pytest.mark.parametrize("k", range(16))
@pytest.mark.parametrize("j", [1, 2])
def test_each_direction_alone(k, j):
    dx, dy = ref.DIRECTIONS[k]
    d = np.full((9, 9), INV)
    d[4 + j * dy, 4 + j * dx] = 6
    assert interp(d)[4, 4] == 6


def test_a_pixel_on_no_ray_is_no_candidate():
    rays = {(4 + j * dy, 4 + j * dx) for dx, dy in ref.DIRECTIONS for j in range(1, 5)}
    off = [(y, x) for y in range(9) for x in range(9) if (y, x) not in rays and (y, x) != (4, 4)]
    assert len(off) == 80 - 4 * 8 - 2 * 8             # 8 rays of 4 pixels, 8 of 2
    for y, x in off:
        d = np.full((9, 9), INV)
        d[y, x] = 6
        stats = {}
        assert interp(d, stats=stats)[4, 4] == INV and stats["no_candidate"] >= 1, (y, x)


def test_the_directions_are_the_sixteen():
    assert len(set(ref.DIRECTIONS)) == 16 and ref.DIRECTIONS[0] == (1, 0) and ref.DIRECTIONS[4] == (0, 1)
    ang = [np.arctan2(dy, dx) % (2 * np.pi) for dx, dy in ref.DIRECTIONS]
    assert ang == sorted(ang)                                            # one turn, from +x towards +y


def test_the_ray_tables_are_the_walk_of_the_definition():
    """vote_ref._nearest_voters (every pixel's ray at once, a step at a time) against the walk of the definition, pixel by pixel
    and direction by direction: a voter mask that is dense, sparse, empty and full, on shapes down to one row and one column"""
    rng = np.random.default_rng(16)
    for h, w, share in ((1, 1, 0.5), (1, 23, 0.3), (17, 1, 0.3), (9, 14, 0.0), (9, 14, 1.0), (23, 31, 0.02), (31, 23, 0.5),
                        (40, 57, 0.1)):
        v = rng.random((h, w)) < share
        near = ref._nearest_voters(v)
        assert len(near) == len(ref.DIRECTIONS)
        for (dx, dy), (qy, qx) in zip(ref.DIRECTIONS, near):
            for y in range(h):
                for x in range(w):
                    py, px, want = y + dy, x + dx, (-1, -1)
                    while 0 <= py < h and 0 <= px < w:
                        if v[py, px]:
                            want = (py, px)
                            break
                        py, px = py + dy, px + dx
                    assert (int(qy[y, x]), int(qx[y, x])) == want, (h, w, share, dx, dy, y, x)


def test_the_first_voter_on_a_ray_is_the_candidate():
    d = np.full((9, 9), INV)
    d[4, 5] = D                     # valid, not a voter: passed over
    d[4, 6] = F32("nan")
    d[4, 7] = 2
    d[4, 8] = 7
    assert interp(d)[4, 4] == 2


def test_an_occlusion_takes_the_largest_candidate():
    d = np.full((9, 9), INV)
    d[4, 6], d[6, 4], d[2, 2], d[4, 0] = 2, 5, 3, F32(4.5)
    assert interp(d)[4, 4] == 5
    dr = np.full((9, 9), F32(50))                                        # no label passes the LR test: still an occlusion
    assert interp(d, disp_r=dr)[4, 4] == 5
    assert interp(d, disp_r=None)[4, 4] == 5
    # the candidate's bits are copied
    d[6, 4] = F32(5.25)
    assert interp(d)[4, 4] == F32(5.25)
    # +0 and -0 are equal values: the first in the order
    z = np.full((9, 9), INV)
    z[4, 6], z[6, 4] = F32(-0.0), F32(0.0)
    assert np.signbit(interp(z)[4, 4])
    z[4, 6], z[6, 4] = F32(0.0), F32(-0.0)
    assert not np.signbit(interp(z)[4, 4])


def test_a_mismatch_takes_the_closest_colour():
    d = np.full((9, 9), INV)
    d[4, 6], d[6, 4], d[2, 2] = 2, 5, 3
    g = GUIDE9.copy()
    g[4, 6], g[6, 4], g[2, 2] = 110, 120, 104
    dr = np.zeros((9, 9), F32)                                           # d = 0: |0 + 0| <= 0 -- every pixel is a mismatch
    stats = {}
    assert interp(d, g, dr, stats=stats)[4, 4] == 3 and stats["mismatch"] >= 1
    assert interp(d, g, None)[4, 4] == 5                                 # disp_r = None: everything an occlusion
    # equal distances: the first in the order of the directions -- (1, 0) before (0, 1) before (-1, -1)
    g[4, 6], g[6, 4], g[2, 2] = 104, 96, 104
    assert interp(d, g, dr)[4, 4] == 2
    g[4, 6] = 105
    assert interp(d, g, dr)[4, 4] == 5
    # colour: the largest channel difference, a fourth byte ignored
    g3 = np.full((9, 9, 4), 100, np.uint8)
    g3[4, 6] = (100, 100, 130, 100)
    g3[6, 4] = (110, 90, 100, 255)
    g3[2, 2] = (120, 100, 100, 100)
    assert interp(d, g3, dr)[4, 4] == 5


def test_no_candidate_leaves_the_pixel_unchanged():
    d = np.full((9, 9), INV)
    d[0, 0] = F32("nan")
    out = interp(d)
    assert np.array_equal(out.view(np.uint32), d.view(np.uint32))
    d[5, 7] = 3                     # (3, 1) from the centre: on none of its rays
    assert interp(d)[4, 4] == INV and interp(d)[5, 4] == 3


@pytest.mark.parametrize("d_lr", [0, 1])
def test_the_mismatch_test_at_the_image_edges(d_lr):
    w = 8
    # labels -3 .. 0: at x = 0 only d = 0 stays inside the image
    dr = np.full((1, w), F32(50))
    assert not ref.mismatch(dr, 0, 0, w, -3, 4, d_lr)
    dr[0, 0] = F32(d_lr)            # |0 + d_lr| <= d_lr
    assert ref.mismatch(dr, 0, 0, w, -3, 4, d_lr)
    dr[0, 0] = F32(d_lr + 1)
    assert not ref.mismatch(dr, 0, 0, w, -3, 4, d_lr)
    dr[0, 0] = F32(-d_lr)
    assert ref.mismatch(dr, 0, 0, w, -3, 4, d_lr)
    # labels 0 .. 3: at x = w - 1 only d = 0; at x = w - 3 also d = 2, which matches -2 on the right
    dr = np.full((1, w), F32(50))
    dr[0, w - 1] = F32(-2 - d_lr)
    assert not ref.mismatch(dr, 0, w - 1, w, 0, 4, d_lr)
    assert ref.mismatch(dr, 0, w - 3, w, 0, 4, d_lr)
    assert not ref.mismatch(dr, 0, w - 3, w, 0, 2, d_lr)                 # (d = 2 is no label of the range)
    dr[0, w - 1] = F32(-2 - d_lr - 1)
    assert not ref.mismatch(dr, 0, w - 3, w, 0, 4, d_lr)
    # a NaN fails the test; a range wholly outside the image has no label to test
    dr[:] = F32("nan")
    assert not ref.mismatch(dr, 0, 3, w, -3, 8, d_lr)
    assert not ref.mismatch(np.zeros((1, w), F32), 0, 3, w, 20, 4, d_lr)
    assert not ref.mismatch(None, 0, 3, w, 0, 4, d_lr)


def test_the_interpolation_reads_a_snapshot():
    """a filled pixel is no candidate of its neighbour in the same pass"""
    d = np.full((1, 9), INV)
    d[0, 0] = 2
    d[0, 8] = 5
    out = ref.interpolate(d, np.full((1, 9), 9, np.uint8), None, 0, D, 0)
    assert (out[0, 1:8] == 5).all()


# ---------------------------------------------------------------------------------------------
# the reason for the feature
# ---------------------------------------------------------------------------------------------
def step_case():
    g, _, truth = cross_ref.step_scene(seed=1)
    d = truth.astype(F32)
    block = (slice(8, 16), slice(24, 32))           # on the surface with the smaller map value, flush against the step
    assert (truth[block] == 2).all() and (truth[:, 32] == 5).all()
    d[block] = INV
    return g, d, truth, block


def test_the_block_beside_the_step():
    """Two textureless surfaces of equal luminance, labels 2 | 5.  An invalidated block of 8 x 8 on the left one, against the
    step: the scan-line fill paints it with the right surface's label (the larger of its two neighbours), the vote of the
    cross regions -- which end at the colour edge -- gives it its own."""
    g, d, truth, block = step_case()
    fill_alone = ref.fill_rows(d, 0)
    voted = ref.region_vote_guide(d, g, None, 0, D, 0, cross=dict(l1=17, l2=8, tau1=20, tau2=6))
    both = ref.fill_rows(voted, 0)
    wrong_fill, wrong_both = int((fill_alone != truth).sum()), int((both != truth).sum())
    print(f"step scene: wrong pixels after the fill alone {wrong_fill}, after voting + fill {wrong_both}")
    assert wrong_fill >= 1 and (fill_alone[block] != truth[block]).any()
    assert wrong_both == 0
    # the vote alone did it: nothing was left to the interpolation or to the fill
    only_vote = ref.region_vote_guide(d, g, None, 0, D, 0, cross=dict(l1=17, l2=8, tau1=20, tau2=6), interpolate_=0)
    assert np.array_equal(only_vote, truth.astype(F32))


# ---------------------------------------------------------------------------------------------
# refusals: no GPU needed
# ---------------------------------------------------------------------------------------------
BAD_PARAMS = [dict(tau_s=-1), dict(tau_h_pct=-1), dict(tau_h_pct=100), dict(iterations=-1), dict(iterations=9),
              dict(interpolate=2), dict(interpolate=-1), dict(tau_s=-5, iterations=20)]
BAD_ARMS = [dict(l1=0), dict(l1=64), dict(l2=35), dict(tau2=0), dict(tau1=5), dict(tau1=257)]


def _params(**kw):
    p = smx.default_vote_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _arms(**kw):
    p = smx.default_cross_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults_and_workspace_size():
    L = smx.lib()
    p = smx.default_vote_params()
    assert (p.tau_s, p.tau_h_pct, p.iterations, p.interpolate) == (20, 40, 5, 1)
    assert ref.params_ok(**ref.DEFAULTS) and ref.DEFAULTS == {k: getattr(p, k) for k in ref.DEFAULTS}
    assert L.smx_vote_workspace_bytes(7, 5) == 255 + 8 * 35
    assert L.smx_vote_workspace_bytes(1, 70000) > 0
    for bad in ((0, 5), (5, 0), (-1, 5), (65536, 32768)):
        assert L.smx_vote_workspace_bytes(*bad) == 0, bad
    tw, th = C.c_int(0), C.c_int(0)
    assert L.smx_vote_geometry(C.byref(tw), C.byref(th)) == 0 and tw.value >= 1 and th.value >= 1
    assert L.smx_vote_geometry(None, C.byref(th)) == -1


def test_every_entry_refuses_invalid_arguments_before_any_device_call():
    L = smx.lib()
    x = C.c_void_p(4096)            # never dereferenced: every call below fails its checks
    wsb = L.smx_vote_workspace_bytes(7, 5)

    def dev(p, arms=x, g=x, ch=3, d=x, dr=x, out=x, w=7, h=5, D=4, ws=x, wsb=wsb):
        return L.smx_dev_region_vote(p, arms, g, ch, d, dr, out, w, h, 0, D, 0, ws, wsb, None)

    def host(p, cross=None, g=x, ch=3, d=x, dr=x, out=x, w=7, h=5, D=4):
        return L.smx_region_vote(p, cross, g, ch, d, dr, out, w, h, 0, D, 0)

    for bad in BAD_PARAMS:
        assert not ref.params_ok(**{**ref.DEFAULTS, **bad}), bad
        p = C.byref(_params(**bad))
        for entry in (dev, host):
            assert entry(p) == -1, (entry.__name__, bad)
            assert b"tau_s" in L.smx_last_error()
        assert L.smx_ctx_set_vote(None, p, None) == -1
    ok = C.byref(_params())
    for entry in (dev, host):
        assert entry(None) == -1
        for kw in (dict(ch=2), dict(ch=0), dict(ch=5), dict(w=0), dict(h=0), dict(w=65536, h=32768), dict(D=0), dict(D=513),
                   dict(d=None), dict(out=None)):
            assert entry(ok, **kw) == -1, (entry.__name__, kw)
    assert not any(ref.shape_ok(*s) for s in ((0, 5, 4), (7, 0, 4), (65536, 32768, 4), (7, 5, 0), (7, 5, 513))) and ref.shape_ok(7, 5, 512)
    assert dev(ok, arms=None) == -1
    assert dev(ok, g=None) == -1                            # the mismatches read it
    assert host(ok, g=None) == -1 and host(ok, g=None, dr=None) == -1        # (the host entry builds the arms from it)
    for bad in BAD_ARMS:
        assert host(ok, cross=C.byref(_arms(**bad))) == -1, bad
        assert b"l1" in L.smx_last_error()
    # the workspace: one byte short, or missing, is SMX_E_WS before anything is launched
    assert dev(ok, wsb=wsb - 1) == -3 and b"workspace" in L.smx_last_error()
    assert dev(ok, ws=None) == -3
    assert L.smx_ctx_set_vote(None, ok, None) == -1 and L.smx_ctx_vote_map(None, None) == -1


def test_the_python_layers_refuse():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    d = np.zeros((5, 7), F32)
    g = np.zeros((5, 7), np.uint8)
    for bad in (dict(disparity=np.zeros((2, 5, 7), F32)), dict(guide=np.zeros((5, 7, 2), np.uint8)), dict(guide=np.zeros((5, 6), np.uint8)),
                dict(disparity_right=np.zeros((5, 6), F32)), dict(params=smx.default_cross_params()), dict(arms=smx.default_vote_params())):
        kw = dict(disparity=d, guide=g, dmin=0, size_d=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            smx.region_vote(**kw)
    for bad in (dict(params=_params(tau_h_pct=100)), dict(arms=_arms(l1=64)), dict(size_d=0), dict(size_d=513)):
        kw = dict(disparity=d, guide=g, dmin=0, size_d=4)
        kw.update(bad)
        with pytest.raises(smx.SmxError) as e:
            smx.region_vote(**kw)
        assert e.value.code == -1
    for kw in (dict(vote="yes"), dict(vote=smx.default_cross_params()), dict(vote=True, vote_arms=smx.default_vote_params()),
               dict(vote_arms=smx.default_cross_params())):
        with pytest.raises(ValueError):
            PairPipeline(64, 24, 8, device="cpu", **kw)
    for kw in (dict(vote=True), dict(vote=smx.default_vote_params()), dict(vote_arms=smx.default_cross_params())):
        with pytest.raises(ValueError, match="region voting"):
            ShardedPair(64, 24, 8, **kw)
    assert isinstance(smx.default_vote_params(), _lib.VoteParams) and smx.VoteParams is _lib.VoteParams
