"""Hierarchical belief propagation without a GPU: the numpy reference (tests/bp_ref.py) against a scalar brute force written
here from the definition in include/smx.h (the direct min over z' of h + V, one message at a time, explicit parity and pyramid
loops), the properties that follow from the definition, the argument checks of the library's host-only entry points, and
what the method buys on the two synthetic scenes of tests/test_perm_cpu.py against references already in the repository.

Measured with this reference (wrong pixels among the kept ones; the draft's figures of the issue in brackets):
  step scene, costs x 16, seeds 0 / 1 / 2:  BP 12 / 15 / 7 (12 / 15 / 7);  best SGM pair 122 / 115 / 121 (122 / 115 / 121)
  step scene, unscaled:                     BP 3 / 8 / 0 (3 / 8 / 0);      SGM at its defaults 19 / 13 / 19 (19 / 13 / 19)
  band scene, unscaled, seeds 0 / 1:        4 levels x 5 iterations 0 / 231 (0 / 231);  1 level x 20 iterations 2128 / 2233
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import bp_ref as ref
import sgm_ref
from test_perm_cpu import band_scene, step_scene

W, H, D, DMINL, DMINR = 192, 48, 16, -15, 0


def brute_force(cost, step, trunc, iterations, levels, data_scale=1.0, messages=None):
    """S by the definition, one scalar at a time.  messages (a list) receives every message of every level after its
    iterations."""
    Dn, h0, w0 = cost.shape
    f32 = np.float32
    sizes = [(w0, h0)]
    for _ in range(levels - 1):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    data = []
    first = {}
    for y in range(h0):
        for x in range(w0):
            col = []
            for z in range(Dn):
                t = f32(cost[z, y, x]) * f32(data_scale)
                col.append((int(t) if t <= 255 else 255) if t >= 0 else 0)
            first[x, y] = col
    data.append(first)
    for l in range(1, levels):
        w, h = sizes[l]
        fw, fh = sizes[l - 1]
        lv = {}
        for y in range(h):
            for x in range(w):
                kids = [(cx, cy) for cy in (2 * y, 2 * y + 1) for cx in (2 * x, 2 * x + 1) if cx < fw and cy < fh]
                lv[x, y] = [sum(data[l - 1][k][z] for k in kids) for z in range(Dn)]
        data.append(lv)
    # msg[p][q]: the message into p from its neighbour q
    msg = None
    for l in range(levels - 1, -1, -1):
        w, h = sizes[l]
        nbrs = lambda x, y: [(x + dx, y + dy) for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)) if 0 <= x + dx < w and 0 <= y + dy < h]
        new = {}
        for y in range(h):
            for x in range(w):
                new[x, y] = {}
                for q in nbrs(x, y):
                    if msg is None:
                        new[x, y][q] = [0] * Dn
                    else:
                        # the parent's message from the same side; from outside the parent's level it is 0
                        side = (q[0] - x, q[1] - y)
                        par = (x >> 1, y >> 1)
                        src = (par[0] + side[0], par[1] + side[1])
                        new[x, y][q] = list(msg[par].get(src, [0] * Dn))
        msg = new
        for t in range(1, iterations + 1):
            fresh = {}
            for y in range(h):
                for x in range(w):
                    if (x + y + t) % 2:
                        continue
                    for q in nbrs(x, y):
                        hq = [data[l][q][z] + sum(msg[q][r][z] for r in nbrs(*q) if r != (x, y)) for z in range(Dn)]
                        m = [min(hq[k] + min(step * abs(z - k), trunc) for k in range(Dn)) for z in range(Dn)]
                        low = min(m)
                        fresh[(x, y), q] = [v - low for v in m]
            for (p, q), m in fresh.items():
                msg[p][q] = m
        if messages is not None:
            messages.extend(v for p in msg.values() for m in p.values() for v in m)
    S = np.zeros((Dn, h0, w0), np.int64)
    for (x, y), col in data[0].items():
        for z in range(Dn):
            S[z, y, x] = col[z] + sum(m[z] for m in msg[x, y].values())
    return S


def _volume(seed, D, h, w, hi=256):
    return np.random.default_rng(seed).integers(0, hi, (D, h, w)).astype(np.float32)


PENALTIES = [(20, 60), (0, 0), (7, 7), (1, 4095), (4095, 4095), (3, 0)]


@pytest.mark.parametrize("levels", [1, 2, 4])
@pytest.mark.parametrize("iterations", [0, 1, 3])
@pytest.mark.parametrize("w,h,D", [(1, 1, 1), (1, 6, 3), (6, 1, 2), (2, 2, 4), (5, 3, 5), (7, 9, 4), (9, 7, 5)])
def test_reference_against_brute_force(w, h, D, iterations, levels):
    for hi in (63, 256):
        cost = _volume(w * 100 + h * 10 + D + hi, D, h, w, hi)
        for step, trunc in PENALTIES:
            got = ref.aggregate(cost, step, trunc, iterations, levels)
            assert np.array_equal(got, brute_force(cost, step, trunc, iterations, levels)), (hi, step, trunc)


def test_data_scale_is_one_f32_product_in_front_of_the_clamp():
    cost = (np.random.default_rng(1).random((5, 4, 6)) * 2.5).astype(np.float32)
    got = ref.aggregate(cost, 20, 60, 3, 2, data_scale=16.0)
    assert np.array_equal(got, brute_force(cost, 20, 60, 3, 2, data_scale=16.0))
    assert ref.clamp(cost, 16.0).max() > 30 and not np.array_equal(ref.clamp(cost, 16.0), 16 * ref.clamp(cost))


def test_no_iterations_and_no_penalties_give_the_clamped_costs():
    cost = _volume(3, 6, 8, 11)
    Cv = ref.clamp(cost)
    assert np.array_equal(ref.aggregate(cost, 20, 60, 0, 4), Cv)
    assert np.array_equal(ref.aggregate(cost, 0, 0, 5, 4), Cv)
    assert np.array_equal(ref.aggregate(cost, 0, 0, 5, 1), Cv)


def test_constant_volume_names_the_last_slice():
    cost = np.full((6, 5, 7), 17, np.float32)
    r = ref.outputs(cost)
    assert (r["S"] == 17).all() and (r["z"] == 5).all()
    assert (r["keys"] == _lib.lib().smx_pack_key(17.0, 5)).all()
    assert np.isnan(r["nbr"][1]).all() and (r["nbr"][0] == 17).all() and (r["nbr"][2] == 17).all()


@pytest.mark.parametrize("step,trunc", PENALTIES)
def test_every_message_of_every_level_lies_in_0_trunc(step, trunc):
    cost = _volume(5, 7, 9, 12)
    trace = []
    ref.run(ref.clamp(cost), step, trunc, 3, 3, trace=trace)
    assert [l for l, _ in trace] == [2, 1, 0]
    for _, M in trace:
        assert M.min() >= 0 and M.max() <= trunc
    seen = []
    brute_force(cost[:4, :5, :6], step, trunc, 2, 3, messages=seen)
    assert min(seen) >= 0 and max(seen) <= trunc


def test_transposing_the_volume_transposes_s():
    cost = _volume(6, 5, 6, 9)
    S = ref.aggregate(cost)
    assert np.array_equal(ref.aggregate(cost.transpose(0, 2, 1).copy()), S.transpose(0, 2, 1))


def test_clamp():
    v = np.array([-1, -0.0, 0.0, 0.99, 1, 254.999, 255, 255.5, 300, np.nan, np.inf, -np.inf, 1e30, -1e-30], np.float32)
    assert ref.clamp(v, 1.0).tolist() == [0, 0, 0, 0, 1, 254, 255, 255, 255, 0, 255, 0, 255, 0]
    assert np.array_equal(ref.clamp(v, 1.0), sgm_ref.clamp(v))
    assert ref.clamp(np.array([1e30, -1e30, 0.124, 0.125], np.float32), 1e30).tolist() == [255, 0, 255, 255]
    assert ref.clamp(np.array([0.124, 0.125, 31.9], np.float32), 8.0).tolist() == [0, 1, 255]


def test_keys_match_the_library_packing():
    r = ref.outputs(_volume(7, 5, 4, 6))
    L = _lib.lib()
    for (y, x), k in np.ndenumerate(r["keys"]):
        assert k == L.smx_pack_key(float(r["best"][y, x]), int(r["z"][y, x]))


# ---- host-only C ABI -------------------------------------------------------------------------------------------------
def _p(step=20, trunc=60, iterations=5, levels=4, data_scale=1.0):
    p = _lib.BpParams()
    p.step, p.trunc, p.iterations, p.levels, p.data_scale = step, trunc, iterations, levels, data_scale
    return p


def test_defaults():
    p = smx.default_bp_params()
    assert (p.step, p.trunc, p.iterations, p.levels, p.data_scale) == (20, 60, 5, 4, 1.0)
    assert isinstance(p, smx.BpParams)


@pytest.mark.parametrize("kw,size_d", [(dict(step=-1), 4), (dict(step=4096), 4), (dict(trunc=-1), 4), (dict(trunc=4096), 4),
                                       (dict(iterations=-1), 4), (dict(iterations=65), 4), (dict(levels=0), 4),
                                       (dict(levels=9), 4), (dict(data_scale=0.0), 4), (dict(data_scale=-1.0), 4),
                                       (dict(data_scale=float("nan")), 4), (dict(data_scale=float("inf")), 4), ({}, 257),
                                       ({}, 0)])
def test_bad_arguments_are_refused_without_a_gpu(kw, size_d):
    L = smx.lib()
    buf = np.zeros(4 * 4 * 8, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p(**kw)
    assert L.smx_dev_bp_wta_pair(C.byref(p), ptr, ptr, 4, 4, size_d, ptr, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_last_error()
    assert L.smx_bp_aggregate(C.byref(p), ptr, None, ptr, ptr, 4, 4, size_d, 0) == -1


def test_null_pointers_shapes_and_a_short_workspace_are_refused_without_a_gpu():
    L = smx.lib()
    buf = np.zeros(64, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = _p()
    args = (4, 4, 4, ptr, None, None, None)
    assert L.smx_dev_bp_wta_pair(None, ptr, ptr, *args, ptr, 1 << 40, None) == -1
    assert L.smx_dev_bp_wta_pair(C.byref(p), None, None, *args, ptr, 1 << 40, None) == -1
    assert L.smx_dev_bp_wta_pair(C.byref(p), ptr, ptr, 4, 4, 4, None, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_dev_bp_wta_pair(C.byref(p), ptr, ptr, 0, 4, 4, ptr, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_dev_bp_wta_pair(C.byref(p), ptr, ptr, 4, 0, 4, ptr, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_dev_bp_wta_pair(C.byref(p), ptr, ptr, 65536, 32768, 4, ptr, None, None, None, ptr, 1 << 40, None) == -1
    assert L.smx_bp_aggregate(None, ptr, None, ptr, ptr, 4, 4, 4, 0) == -1
    assert L.smx_bp_aggregate(C.byref(p), None, None, ptr, ptr, 4, 4, 4, 0) == -1
    for l, r, nviews in ((ptr, ptr, 2), (ptr, None, 1), (None, ptr, 1)):
        need = L.smx_bp_workspace_bytes(4, 4, 4, 4, nviews)
        assert need > 0
        assert L.smx_dev_bp_wta_pair(C.byref(p), l, r, *args, ptr, need - 1, None) == -3
        assert L.smx_dev_bp_wta_pair(C.byref(p), l, r, *args, None, need, None) == -3
        assert b"workspace" in L.smx_last_error()
    with pytest.raises(ValueError):
        smx.bp_aggregate(np.zeros((4, 4), np.float32))


def _formula(w, h, d, levels, nviews):
    """include/smx.h: 255 + nviews * (A(2 n_0 Dp) + sum_l (A((l ? 4 : 1) n_l Dp) + A(8 n_l Dp)))"""
    A = lambda b: (b + 255) // 256 * 256
    dp = (d + 63) // 64 * 64
    view = A(2 * w * h * dp)
    for l in range(levels):
        view += A((4 if l else 1) * w * h * dp) + A(8 * w * h * dp)
        w, h = (w + 1) // 2, (h + 1) // 2
    return 255 + nviews * view


def test_workspace_bytes():
    ws = smx.lib().smx_bp_workspace_bytes
    assert ws(0, 5, 4, 4, 1) == 0 and ws(5, 0, 4, 4, 1) == 0 and ws(5, 5, 0, 4, 1) == 0 and ws(5, 5, 257, 4, 1) == 0
    assert ws(5, 5, 4, 0, 1) == 0 and ws(5, 5, 4, 9, 1) == 0 and ws(5, 5, 4, 4, 0) == 0 and ws(5, 5, 4, 4, 3) == 0
    assert ws(65536, 32768, 4, 4, 1) == 0
    assert ws(5, 5, 256, 8, 2) > 0
    for w, h, d, lv, v in ((1, 1, 1, 1, 1), (7, 5, 9, 1, 1), (7, 5, 9, 4, 2), (64, 64, 64, 3, 1), (129, 70, 70, 4, 2),
                           (33, 6, 255, 8, 1), (1242, 375, 192, 4, 2)):
        assert ws(w, h, d, lv, v) == _formula(w, h, d, lv, v)
        assert ws(w + 1, h, d, lv, v) >= ws(w, h, d, lv, v) and ws(w, h + 1, d, lv, v) >= ws(w, h, d, lv, v)
        assert ws(w, h, d + 1, lv, v) >= ws(w, h, d, lv, v)
        if lv < 8:
            assert ws(w, h, d, lv + 1, v) > ws(w, h, d, lv, v)
        if v == 1:
            assert ws(w, h, d, lv, 2) > ws(w, h, d, lv, 1)
    assert all(ws(9, 9, d + 1, 4, 1) >= ws(9, 9, d, 4, 1) for d in range(1, 256))
    # about 11 bytes per cell at level 0 and a third of 12 more above it: about 1 GB a view at the KITTI shape
    cells = 1242 * 375 * 192
    assert 14.9 * cells <= ws(1242, 375, 192, 4, 1) <= 15.0 * cells


# ---- what it buys ----------------------------------------------------------------------------------------------------
KEEP = np.ones(W, bool)
KEEP[:20] = False


def _wrong(z, truth, keep):
    return int(((DMINL + z) != truth)[:, keep].sum())


SGM_PAIRS = [(10, 120), (20, 60), (2, 8), (40, 400), (5, 30)]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_step_scene_against_sgm(seed):
    """BP at its defaults, times 4, is at most the best of five SGM penalty pairs (8 paths) on the costs x 16."""
    import oracle
    L, R, truth = step_scene(seed)
    cost = oracle.stereo_pair(L, R, D, dminl=DMINL, dminr=DMINR, want_cost=True)["costl"]
    keep = KEEP.copy()
    keep[74:80] = False                 # occluded in the right view: nothing is asserted inside
    assert int(keep.sum()) * H == 7968
    scaled = (cost * np.float32(16)).astype(np.float32)
    sgm = {pp: _wrong(sgm_ref.outputs(scaled, pp[0], pp[1], 8)["z"], truth, keep) for pp in SGM_PAIRS}
    zb = ref.outputs(cost, data_scale=16.0)["z"]
    assert np.array_equal(zb, ref.outputs(scaled)["z"])
    bp = _wrong(zb, truth, keep)
    plain_sgm = _wrong(sgm_ref.outputs(cost)["z"], truth, keep)
    plain_bp = _wrong(ref.outputs(cost)["z"], truth, keep)
    print(f"seed {seed}: step scene x 16: BP {bp} wrong of 7968, SGM {sgm}; inside the occluded columns BP",
          int(((DMINL + zb) != truth)[:, 74:80].sum()), f"of {6 * H} | unscaled: BP {plain_bp}, SGM at its defaults {plain_sgm}")
    assert 4 * bp <= min(sgm.values())


@pytest.mark.parametrize("seed", [0, 1])
def test_band_scene_the_pyramid_carries_information_across_the_band(seed):
    """4 levels x 5 iterations, times 4, is at most 1 level x 20 iterations (the same number of level-0 sweeps and more)."""
    import oracle
    d = 6
    L, R = band_scene(seed, d, 60)
    cost = oracle.stereo_pair(L, R, D, dminl=DMINL, dminr=DMINR, want_cost=True)["costl"]
    truth = np.full((H, W), -float(d))
    assert int(KEEP.sum()) * H == 8256
    pyr = _wrong(ref.outputs(cost, 20, 60, 5, 4)["z"], truth, KEEP)
    flat = _wrong(ref.outputs(cost, 20, 60, 20, 1)["z"], truth, KEEP)
    print(f"seed {seed}: band scene: 4 levels x 5 iterations {pyr} wrong of 8256, 1 level x 20 iterations {flat}")
    assert 4 * pyr <= flat


def test_pipeline_and_sharded_driver_refuse_what_they_do_not_take():
    from stereo_matching_cuda_amd.device import PairPipeline
    from stereo_matching_cuda_amd.sharded import ShardedPair
    with pytest.raises(ValueError, match="belief propagation"):
        ShardedPair(16, 8, 4, aggregation="bp")
    with pytest.raises(ValueError):
        PairPipeline(16, 8, 257, aggregation="bp")
    with pytest.raises(ValueError):
        PairPipeline(16, 8, 4, aggregation="bp", s_begin=0, s_end=2)
    with pytest.raises(ValueError):
        PairPipeline(16, 8, 4, aggregation="bp", bp_params=_p(step=4096))
