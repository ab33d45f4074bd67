"""The fused walkers at the edges of the parameter and cost gates, against the oracle (bit-exact) and the multi-kernel path.

One table of parameter points built from the boundaries of the gates (smx_debug_agg_path, tests/test_agg_gate.py): alpha,
the thresholds and eps on each side of what the comb walker and the ring walker admit, at radius 8 and 9.  The images put
pixel values of 255 and derivatives of +-127.5 within the disparity range of both image edges, where every partner of a
range that leaves the image on both sides is the sentinel cell, so a walker whose out-of-range cost is not the reference's
border constant cannot pass.  Then the materialised-cost convention at the bounds of the comb walker's value check
([2^-60, 2^60]), with the queued fall-back over several chunks.

Run on the GPU box:  python -m pytest tests -m gpu -q
"""
import ctypes as C
import math

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from test_agg_gate import INT_MAX, hook, params
from test_gpu_parity import KEYS, _device_pair, _eq, _fallback_ran, _geometry

pytestmark = pytest.mark.gpu

D = 24
DMINL, DMINR = -12, -11          # both views: partners leave the image on the left and on the right


@pytest.fixture(scope="module")
def so():
    smx.lib()                    # first: binds the library to torch's HIP runtime (_lib._preload_torch_hip_runtime)
    L = C.CDLL(smx._lib.SO_PATH)
    L.smx_debug_agg_path.restype = C.c_int
    L.smx_debug_agg_path.argtypes = [C.POINTER(smx.Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.smx_last_error.restype = C.c_char_p
    return L


def _shape():
    """Two strips plus a ragged one, two bands plus a remainder, of the comb walker (smx_agg_geometry); ragged for the ring
    walker too."""
    ow, bh, _ = _geometry(9)
    w, h = 2 * ow + ow // 4, 2 * bh + bh // 2
    assert w % 64 and h % 16 and w % ow and h % bh
    return w, h


def _edge_images():
    w, h = _shape()
    rng = np.random.default_rng(4242)
    base = rng.integers(0, 256, size=(h, w + 16), dtype=np.uint8)
    ims = [np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, 5:5 + w])]
    # (255, 255, 0, 0) repeated: pixel values 255 and derivatives (I[x-1] - I[x+1]) / 2 = +127.5 / -127.5, in the first and
    # last D columns (every row of the top band, every other row below) of both guides
    pat = np.resize(np.array([255, 255, 0, 0], np.uint8), D)
    for k, im in enumerate(ims):
        for y in range(h):
            if y < 10 or y % 2 == k:
                im[y, :D] = np.roll(pat, y % 4)
                im[y, w - D:] = np.roll(pat, (y + 1) % 4)
        im[h - 9:h - 2, 120:200] = 77      # a flat region in both views: exact zero costs and ties between slices
    return ims


_ALPHA = [0.0, 1.0, 2.0**-59, float(np.nextafter(np.float32(2.0**-59), np.float32(0))), 0.3, 1 / 3, -1e-50, 1 + 1e-12]
_THC = [0, 1, 255, 256, 2048, 2049, 59744, 59776, 59968, 60000, 65535, INT_MAX]
_THG = [0, 1, 127, 128, 59872, 59904, 60000, INT_MAX]
_EPS = [math.nextafter(1.0, 0.0), 1.0, 6.5025, 1e29, math.nextafter(1e30, 0.0), 1e30]
_POINTS = ([("alpha", a) for a in _ALPHA] + [("th_color", t) for t in _THC] + [("th_grad", t) for t in _THG] +
           [("eps", e) for e in _EPS] + [("denormal", None)])


def _point(radius, name, value):
    if name == "denormal":     # alpha at the comb walker's smallest, costs 2^-60 apart, eps large: the a_k come out denormal
        return params(radius=radius, alpha=2.0**-59, th_color=0, eps=1e29)
    return params(radius=radius, **{name: value})


@pytest.fixture(scope="module")
def edge_images():
    return _edge_images()


@pytest.mark.parametrize("radius", [8, 9])
@pytest.mark.parametrize("name,value", _POINTS, ids=[f"{n}={v!r}" for n, v in _POINTS])
def test_gate_point_is_bit_exact(orc, so, edge_images, radius, name, value):
    Il, Ir = edge_images
    h, w = Il.shape
    p = _point(radius, name, value)
    want = orc.stereo_pair(Il, Ir, D, dminl=DMINL, dminr=DMINR, want_agg=True, params=orc.Params.from_buffer_copy(bytes(p)))
    auto, _ = hook(so, p, w, h, 2, False, 0)
    runs = [(0, auto), (1, 1)] + ([(3, 2)] if auto == 5 else [])     # path 3: the ring walker where both walkers apply
    for path, ran in runs:
        r = _device_pair(Il, Ir, D, path=path, dminl=DMINL, dminr=DMINR, want_agg=True, params=p)
        assert smx.lib().smx_last_agg_path() == ran, (path, ran)
        for k in KEYS + ("aggl", "aggr"):
            _eq(r[k], want[k], f"path {path} (ran {ran}) {k}")


@pytest.mark.parametrize("thc,thg", [(59746, 2), (7, 59873), (INT_MAX, 2)])
def test_forced_walker_refuses_thresholds_beyond_the_sentinel(edge_images, thc, thg):
    """A fused path forced with thresholds the sentinel cannot saturate is an argument error naming the reason, not a wrong
    border cost; the same parameters on the default path run the multi-kernel path."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir = edge_images
    h, w = Il.shape
    p = params(th_color=thc, th_grad=thg)
    dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    for path in (2, 3, 4, 5):
        pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, params=p)
        smx.lib().smx_set_agg_path(path)
        try:
            with pytest.raises(smx.SmxError, match="th_color > 59745 or th_grad > 59872") as e:
                pipe.aggregate(dl, dr)
            assert e.value.code == -1
        finally:
            smx.lib().smx_set_agg_path(0)
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, params=p)
    pipe.run(dl, dr)
    assert smx.lib().smx_last_agg_path() == 1


# ---- materialised cost volumes --------------------------------------------------------------------------------------
F32_MIN = float(np.finfo(np.float32).tiny)
LO, HI = 2.0**-60, 2.0**60
LO_OUT = float(np.nextafter(np.float32(LO), np.float32(0)))
HI_OUT = float(np.nextafter(np.float32(HI), np.float32(np.inf)))


@pytest.fixture(scope="module")
def cost_case(orc, edge_images):
    Il, Ir = edge_images
    return Il, Ir, orc.cost_volume(Il, Ir, D, DMINL), orc.cost_volume(Ir, Il, D, DMINR)


def _view_oracle(orc, I, cost, dmin):
    best, dmap, mean, agg = orc.guided_filter(I, cost, dmin, want_agg=True)
    return orc.pack_keys(best, (dmap - dmin).astype(np.int64)), mean, agg


def _run_cost(Il, Ir, cl, cr, nviews, want_agg, sif=None):
    """The device-pointer calls on materialised volumes: one view (smx_dev_aggregate_wta) or the pair
    (smx_dev_aggregate_wta_pair_cost).  Returns the pipeline (keys / means / volumes on the device) and the fall-back report."""
    import torch
    from stereo_matching_cuda_amd.device import PairPipeline
    h, w = Il.shape
    pipe = PairPipeline(w, h, D, dminl=DMINL, dminr=DMINR, want_agg=want_agg, slices_in_flight=sif)
    dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    if nviews == 1:
        pipe.init_keys()
        pipe.aggregate_view(0, dl, dr, torch.from_numpy(cl).cuda())
    else:
        pipe.aggregate(dl, dr, torch.from_numpy(cl).cuda(), torch.from_numpy(cr).cuda())
    assert smx.lib().smx_last_agg_path() == 5
    pipe.check_status()
    return pipe, _fallback_ran(pipe)


def _check_cost_run(orc, pipe, Il, Ir, cl, cr, nviews, want_agg, what):
    for v, (I, c, dmin) in enumerate(((Il, cl, DMINL), (Ir, cr, DMINR))[:nviews]):
        keys, mean, agg = _view_oracle(orc, I, c, dmin)
        _eq(pipe.keys[v].cpu().numpy(), keys, f"{what} view {v} keys")
        _eq(pipe.mean[v].cpu().numpy(), mean, f"{what} view {v} mean")
        if want_agg:
            _eq(pipe.agg[v].cpu().numpy(), agg, f"{what} view {v} agg")


@pytest.mark.parametrize("values,falls_back", [((LO, HI), False), ((LO_OUT,), True), ((HI_OUT,), True), ((F32_MIN,), True)],
                         ids=["2^-60 and 2^60", "below 2^-60", "above 2^60", "FLT_MIN"])
def test_single_cost_values_at_the_check_bounds(orc, cost_case, values, falls_back):
    """The comb walker's value check admits +0 and the normal numbers in [2^-60, 2^60], bounds included: no fall-back there,
    the f32 neighbours just outside and FLT_MIN raise it.  Exact either way, on the device-pointer and host-pointer calls."""
    Il, Ir, cl, cr = cost_case
    h, w = Il.shape
    cl, cr = cl.copy(), cr.copy()
    for k, v in enumerate(values):           # an interior strip of one slice, the last cell of another
        cl[3 + 7 * k, 12, 160] = np.float32(v)
        cr[D - 1 - k, h - 1, w - 1] = np.float32(v)
    for nviews in (1, 2):
        pipe, fb = _run_cost(Il, Ir, cl, cr, nviews, want_agg=True)
        assert fb == falls_back, (values, nviews)
        _check_cost_run(orc, pipe, Il, Ir, cl, cr, nviews, True, f"{values} nviews={nviews}")
    b1, d1, m1, a1 = orc.guided_filter(Il, cl, DMINL, want_agg=True)
    b2, d2 = smx.init_wta(h, w)
    m2, a2 = smx.compute_guided_filter(Il, cl, b2, d2, DMINL, want_agg=True)
    assert smx.lib().smx_last_agg_path() == 5
    for name, a, b in (("best", b2, b1), ("dmap", d2, d1), ("mean", m2, m1), ("agg", a2, a1)):
        _eq(a, b, f"compute_guided_filter {values} {name}")


@pytest.mark.parametrize("scale", ["2^-60", "2^60"])
def test_whole_volumes_at_the_check_bounds(orc, cost_case, scale):
    """Every cost at the scale of a bound of the value check (and +0 where the reference's cost is zero): the comb walker's
    own argument, no fall-back, bit-exact -- sums, means and the a_k / b_k at the extremes of the admitted range."""
    Il, Ir, _, _ = cost_case
    rng = np.random.default_rng(60)
    vols = []
    for v in range(2):
        m = rng.random((D, *Il.shape))
        c = (LO * (1 + 7 * m)) if scale == "2^-60" else (HI / 8 * (1 + 7 * m))
        c = c.astype(np.float32)
        c[m < 0.1] = 0.0
        assert c.max() <= HI and c[c > 0].min() >= LO
        vols.append(c)
    for nviews in (1, 2):
        pipe, fb = _run_cost(Il, Ir, vols[0], vols[1], nviews, want_agg=True)
        assert not fb, (scale, nviews)
        _check_cost_run(orc, pipe, Il, Ir, vols[0], vols[1], nviews, True, f"{scale} nviews={nviews}")


@pytest.mark.parametrize("nviews", [1, 2])
@pytest.mark.parametrize("want_agg", [True, False])
@pytest.mark.parametrize("where", ["first", "last"])
def test_fallback_over_several_chunks(orc, cost_case, nviews, want_agg, where):
    """slices_in_flight < D: the walker runs chunk by chunk and the queued ring walker redoes every chunk from the one whose
    check failed.  A bad value only in the first chunk or only in the last must still give the oracle's result, with or
    without the caller's aggregated volume; then a clean call on the same workspace reports no fall-back."""
    Il, Ir, cl, cr = cost_case
    h, w = Il.shape
    sif = 5
    bad_l, bad_r = cl.copy(), cr.copy()
    z = 1 if where == "first" else D - 2                 # chunks of 5 slices: [0, 5) ... [20, 24)
    bad_l[z, 7, 200] = np.float32(-0.75)
    bad_r[z, h - 1, 0] = np.float32(2.0**-70)
    pipe, fb = _run_cost(Il, Ir, bad_l, bad_r, nviews, want_agg, sif=sif)
    assert pipe.last_chunk() == (sif, math.ceil(D / sif))
    assert fb, (where, nviews, want_agg)
    _check_cost_run(orc, pipe, Il, Ir, bad_l, bad_r, nviews, want_agg, f"bad in the {where} chunk")
    # the report belongs to the call: a clean call on the same workspace clears it
    import torch
    dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    if nviews == 1:
        pipe.init_keys()
        pipe.aggregate_view(0, dl, dr, torch.from_numpy(cl).cuda())
    else:
        pipe.aggregate(dl, dr, torch.from_numpy(cl).cuda(), torch.from_numpy(cr).cuda())
    assert not _fallback_ran(pipe)
    _check_cost_run(orc, pipe, Il, Ir, cl, cr, nviews, want_agg, "clean call after a bad one")
