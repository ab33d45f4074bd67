"""The ZNCC window matching cost on the GPU (smx_dev_zncc_moments, smx_dev_zncc_cost_pair, smx_zncc_cost,
device.zncc_cost_volumes, smx_ctx_set_zncc).  The two kernels are held to tests/zncc_ref.py bit for bit; everything behind them
to the oracle and to tests/sgm_ref.py fed with the reference's volumes.  All comparisons are equality.

k_zncc_cost_pair works on tiles of smx_zncc_geometry() columns x rows and 16 slices: the shapes aim at those seams.

Run on the GPU box:  python -m pytest tests -m gpu -q -k zncc
"""
import ctypes as C

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

import sgm_ref
import zncc_ref as ref
from guarded import Guarded

pytestmark = pytest.mark.gpu

WINDOWS = [(1, 1), (1, 4), (4, 1), (4, 4), (3, 3)]
MAPS = ("bestl", "bestr", "dmapl", "dmapr", "meanl", "meanr", "occlusion", "filled")
F32 = np.float32


def _eq(a, b, name=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = np.flatnonzero(a.ravel() != b.ravel())
    assert bad.size == 0, f"{name}: {bad.size} of {a.size} elements differ, first at {bad[:5]}"


def _zp(rx=3, ry=3):
    p = _lib.ZnccParams()
    p.rx, p.ry = rx, ry
    return p


def _dp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _geometry():
    cols, rows = C.c_int(), C.c_int()
    _lib.check(smx.lib().smx_zncc_geometry(C.byref(cols), C.byref(rows)))
    return cols.value, rows.value


def _moments(imgs, p):
    """The moments of a pair, one launch for both images -> (images tensor, moments tensor (2, h, w) int64)."""
    import torch
    d = torch.from_numpy(np.stack(imgs)).cuda()
    _, h, w = d.shape
    mom = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    _lib.check(smx.lib().smx_dev_zncc_moments(C.byref(p), _dp(d), _dp(mom), w, h, 2, _stream()))
    return d, mom


def _cost_pair(Il, Ir, p, dminl, dminr, s0, s1, left=True, right=True):
    """smx_dev_zncc_cost_pair -> (left volume or None, right volume or None) as numpy, each with a guard plane behind it that
    must stay untouched."""
    import torch
    d, mom = _moments((Il, Ir), p)
    h, w = Il.shape
    out = [torch.full((s1 - s0 + 1, h, w), -7.0, device="cuda") if on else None for on in (left, right)]
    _lib.check(smx.lib().smx_dev_zncc_cost_pair(C.byref(p), _dp(mom), _dp(d[0]), _dp(d[1]), _dp(out[0]), _dp(out[1]), w, h,
                                                dminl, dminr, s0, s1, _stream()))
    res = []
    for t in out:
        if t is None:
            res.append(None)
            continue
        a = t.cpu().numpy()
        assert np.all(a[-1] == -7.0), "the launch wrote behind its slices"
        res.append(a[:-1])
    return res


def _images(kind, w, h, seed=0):
    """A pair (h, w) uint8: random, constant, two-valued, or the extreme of the 32-bit bounds (all 255 against a 0 / 255
    checkerboard)."""
    rng = np.random.default_rng(100 + seed)
    if kind == "random":
        return tuple(rng.integers(0, 256, (2, h, w), dtype=np.uint8))
    if kind == "constant":
        return np.full((h, w), 77, np.uint8), np.full((h, w), 201, np.uint8)
    if kind == "two-valued":
        return tuple((rng.integers(0, 2, (2, h, w)) * 215 + 20).astype(np.uint8))
    assert kind == "extreme"
    yy, xx = np.mgrid[0:h, 0:w]
    return np.full((h, w), 255, np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8)


def _check_pair(Il, Ir, rx, ry, D, dminl, dminr, s0=0, s1=None, name=""):
    s1 = D if s1 is None else s1
    gl, gr = _cost_pair(Il, Ir, _zp(rx, ry), dminl, dminr, s0, s1)
    _eq(gl, ref.zncc_cost(Il, Ir, D, dminl, rx, ry, s0, s1), f"{name} left")
    _eq(gr, ref.zncc_cost(Ir, Il, D, dminr, rx, ry, s0, s1), f"{name} right")
    return gl, gr


@pytest.mark.parametrize("rx,ry", WINDOWS)
@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 9), (129, 70)])
def test_moments(w, h, rx, ry):
    Il, Ir = _images("random", w, h)
    _, mom = _moments((Il, Ir), _zp(rx, ry))
    got = mom.cpu().numpy().view(np.uint64)
    _eq(got[0], ref.moment_words(Il, rx, ry), "left moments")
    _eq(got[1], ref.moment_words(Ir, rx, ry), "right moments")


def test_moments_one_image_per_launch():
    import torch
    Il, Ir = _images("random", 70, 19, 1)
    p = _zp()
    d = torch.from_numpy(np.stack([Il, Ir])).cuda()
    mom = torch.zeros((2, 19, 70), dtype=torch.int64, device="cuda")
    for v in range(2):
        _lib.check(smx.lib().smx_dev_zncc_moments(C.byref(p), _dp(d[v]), _dp(mom[v]), 70, 19, 1, _stream()))
    _eq(mom.cpu().numpy(), _moments((Il, Ir), p)[1].cpu().numpy(), "moments")


@pytest.mark.parametrize("kind", ["random", "constant", "two-valued", "extreme"])
@pytest.mark.parametrize("w,h,rx,ry,D", [(1, 1, 3, 3, 3), (3, 2, 4, 4, 4), (65, 9, 3, 3, 5)])
def test_small_shapes(w, h, rx, ry, D, kind):
    Il, Ir = _images(kind, w, h)
    gl, _ = _check_pair(Il, Ir, rx, ry, D, -(D - 1), 0, name=f"{w}x{h} {kind}")
    if kind == "constant":
        assert set(np.unique(gl)) <= {128.0, 255.0}


def test_tile_seams():
    """Widths at cols - 1, cols, cols + 1 and 2 cols + 1, heights at rows - 1, rows + 1 and 2 rows + 1, and 18 slices: one past
    the slices of a workgroup."""
    cols, rows = _geometry()
    for i, (w, h) in enumerate([(cols - 1, rows - 1), (cols, rows + 1), (cols + 1, rows - 1), (2 * cols + 1, 2 * rows + 1)]):
        Il, Ir = _images("random", w, h, i)
        _check_pair(Il, Ir, 3, 3, 18, -9, -8, name=f"{w}x{h}")


@pytest.mark.parametrize("rx,ry", WINDOWS)
@pytest.mark.parametrize("kind", ["random", "two-valued", "extreme"])
def test_windows(rx, ry, kind):
    cols, rows = _geometry()
    Il, Ir = _images(kind, cols + 5, rows + 3, rx + ry)
    _check_pair(Il, Ir, rx, ry, 7, -4, -2, name=f"{kind} {rx},{ry}")


@pytest.mark.parametrize("dminl,dminr,D", [(-40, 30, 17), (-37, -37, 4), (37, 37, 3), (-1000, 1000, 3), (-36, 34, 2)])
def test_partners_that_leave_the_image(dminl, dminr, D):
    """Partners outside on the left, on the right, and on every column (|dmin| >= w, the whole volume 255)."""
    w, h = 37, 11
    Il, Ir = _images("random", w, h, D)
    gl, gr = _check_pair(Il, Ir, 2, 3, D, dminl, dminr, name=f"dmin {dminl},{dminr}")
    if dminl in (37, -1000):
        assert np.all(gl == 255.0) and np.all(gr == 255.0)
    else:
        assert np.any(gl == 255.0) and np.any(gl != 255.0)


@pytest.mark.parametrize("s0,s1", [(3, 20), (1, 2), (16, 17), (5, 5)])
def test_slice_sub_ranges(s0, s1):
    Il, Ir = _images("random", 70, 13, s0)
    _check_pair(Il, Ir, 3, 2, 23, -11, -3, s0, s1, name=f"[{s0},{s1})")


def test_single_view_forms_and_the_host_entry():
    w, h, D = 131, 35, 19
    Il, Ir = _images("random", w, h, 3)
    p = _zp(4, 2)
    wl = ref.zncc_cost(Il, Ir, D, -(D - 1), 4, 2)
    wr = ref.zncc_cost(Ir, Il, D, 0, 4, 2)
    gl, none = _cost_pair(Il, Ir, p, -(D - 1), 0, 0, D, right=False)
    assert none is None
    _eq(gl, wl, "left only")
    none, gr = _cost_pair(Il, Ir, p, -(D - 1), 0, 0, D, left=False)
    assert none is None
    _eq(gr, wr, "right only")
    _eq(smx.zncc_cost(Il, Ir, D, -(D - 1), p), wl, "smx_zncc_cost, left")
    _eq(smx.zncc_cost(Ir, Il, D, 0, p), wr, "smx_zncc_cost, right")
    L = smx.lib()
    d, mom = _moments((Il, Ir), p)
    assert L.smx_dev_zncc_cost_pair(C.byref(p), _dp(mom), _dp(d[0]), _dp(d[1]), None, None, w, h, 0, 0, 0, D, _stream()) == -1
    assert L.smx_dev_zncc_cost_pair(C.byref(_zp(5, 1)), _dp(mom), _dp(d[0]), _dp(d[1]), _dp(mom), None, w, h, 0, 0, 0, D, _stream()) == -1
    assert L.smx_dev_zncc_moments(C.byref(_zp(0, 1)), _dp(d), _dp(mom), w, h, 2, _stream()) == -1


def test_invariance_under_a_local_affine_change():
    """B = a A + b with a > 0 gives the volume of A against itself wherever the windows are not clipped: the cost is exactly 0
    at the true label for any gain and offset that keep the values inside 0 .. 255 and apart."""
    A = (_images("random", 90, 20, 9)[0] // 4).astype(np.uint8)
    B = (3 * A.astype(np.int64) + 17).astype(np.uint8)
    got = smx.zncc_cost(A, B, 1, 0)
    assert np.all(got == 0.0)


@pytest.mark.parametrize("shifted", [False, True])
def test_memory_contract(shifted):
    """Every buffer of the two launches inside the guarded, poisoned allocations of tests/guarded.py: the launches write the
    moments and their slices, nothing else, and leave their inputs as they were."""
    cols, rows = _geometry()
    w, h, D, s0, s1 = cols + 3, rows + 2, 19, 2, 19
    Il, Ir = _images("random", w, h, 11)
    p = _zp()

    def guard(array):
        a = np.ascontiguousarray(array)
        return Guarded(a.nbytes, a.dtype, a.shape, plane=w * h).load(a)

    def out(dtype, shape):
        dtype = np.dtype(dtype)
        return Guarded(int(np.prod(shape)) * dtype.itemsize, dtype, shape, misalign=dtype.itemsize if shifted else 0, plane=w * h)

    imgs = guard(np.stack([Il, Ir]))
    mom = out(np.uint64, (2, h, w))
    _lib.check(smx.lib().smx_dev_zncc_moments(C.byref(p), imgs.ptr, mom.ptr, w, h, 2, _stream()))
    mom.check("moments")
    imgs.check_unchanged("images behind the moments")
    words = mom.numpy().view(np.uint64)
    _eq(words[0], ref.moment_words(Il), "left moments")
    mom_in = guard(words)
    cl, cr = out(F32, (s1 - s0, h, w)), out(F32, (s1 - s0, h, w))
    n = w * h
    _lib.check(smx.lib().smx_dev_zncc_cost_pair(C.byref(p), mom_in.ptr, imgs.ptr, C.c_void_p(imgs.ptr.value + n), cl.ptr, cr.ptr,
                                                w, h, -9, -4, s0, s1, _stream()))
    cl.check("left volume")
    cr.check("right volume")
    imgs.check_unchanged("images behind the cost")
    mom_in.check_unchanged("moments behind the cost")
    _eq(cl.numpy(), ref.zncc_cost(Il, Ir, D, -9, 3, 3, s0, s1), "left volume")
    _eq(cr.numpy(), ref.zncc_cost(Ir, Il, D, -4, 3, 3, s0, s1), "right volume")


# ---------------------------------------------------------------------------------------------
# end to end: the pipeline and the context against the oracle fed with the reference's volumes
# ---------------------------------------------------------------------------------------------
W, H, D = 129, 70, 16
DMINL, DMINR = -(D - 1), 0


@pytest.fixture(scope="module")
def scene(orc):
    Il, Ir = synth.gen_pair(W, H, D, W + H)
    cl, cr = ref.zncc_cost(Il, Ir, D, DMINL), ref.zncc_cost(Ir, Il, D, DMINR)
    bl, ml, meanl, aggl = orc.guided_filter(Il, cl, DMINL, want_agg=True)
    br, mr, meanr, aggr = orc.guided_filter(Ir, cr, DMINR, want_agg=True)
    occ = orc.detect_occlusion(ml, mr, DMINL - 100)
    e = dict(costl=cl, costr=cr, bestl=bl, bestr=br, dmapl=ml, dmapr=mr, meanl=meanl, meanr=meanr, aggl=aggl, aggr=aggr,
             occlusion=occ, filled=orc.fill_occlusion(occ, float(DMINL)))
    return Il, Ir, e


def _device_volumes(Il, Ir):
    import torch
    from stereo_matching_cuda_amd.device import zncc_cost_volumes
    imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
    cl, cr = zncc_cost_volumes(imgs[0], imgs[1], D, DMINL, DMINR)
    return imgs, cl, cr


def test_pipeline_with_the_zncc_volumes(scene):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir, e = scene
    imgs, cl, cr = _device_volumes(Il, Ir)
    _eq(cl.cpu().numpy(), e["costl"], "costl")
    _eq(cr.cpu().numpy(), e["costr"], "costr")
    pipe = PairPipeline(W, H, D, dminl=DMINL, dminr=DMINR, want_agg=True)
    pipe.aggregate(imgs[0], imgs[1], cost_l=cl, cost_r=cr)
    pipe.finish()
    r = pipe.results()
    for k in MAPS + ("aggl", "aggr"):
        _eq(r[k], e[k], k)
    assert len(np.unique(e["dmapl"])) > 3 and (e["occlusion"] == DMINL - 100).any()
    rr = C.c_int(-1)                             # integers 0 .. 255: the comb walker's check never fires
    _lib.check(smx.lib().smx_dev_agg_fallback(_dp(pipe.ws), C.byref(rr)))
    assert rr.value == 0


def test_sgm_from_the_zncc_volumes(scene):
    from stereo_matching_cuda_amd.device import PairPipeline
    Il, Ir, e = scene
    imgs, cl, cr = _device_volumes(Il, Ir)
    pipe = PairPipeline(W, H, D, dminl=DMINL, dminr=DMINR, aggregation="sgm", want_agg=True)
    pipe.aggregate(imgs[0], imgs[1], cost_l=cl, cost_r=cr)
    pipe.finish()
    got = pipe.results()
    sl, sr = sgm_ref.outputs(e["costl"]), sgm_ref.outputs(e["costr"])
    _eq(pipe.keys.cpu().numpy(), np.stack([sl["keys"], sr["keys"]]), "keys")
    _eq(got["aggl"], sl["agg"], "aggl")
    _eq(got["aggr"], sr["agg"], "aggr")
    _eq(got["dmapl"], (DMINL + sl["z"]).astype(F32), "dmapl")
    _eq(got["dmapr"], (DMINR + sr["z"]).astype(F32), "dmapr")


def test_context(orc, scene):
    Il, Ir, e = scene
    plain = orc.stereo_pair(Il, Ir, D, dminl=DMINL, dminr=DMINR, want_cost=True)
    L = smx.lib()
    P = smx.default_params()
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(P), W, H, D, C.byref(ctx)))
    try:
        names = {"best_l": "bestl", "best_r": "bestr", "dmap_l": "dmapl", "dmap_r": "dmapr", "occlusion": "occlusion",
                 "filled": "filled", "mean_l": "meanl", "mean_r": "meanr", "cost_l": "costl", "cost_r": "costr",
                 "agg_l": "aggl", "agg_r": "aggr"}

        def run(fields):
            bufs = {k: np.empty(e[names[k]].shape, e[names[k]].dtype) for k in fields}
            out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
            _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)))
            return bufs

        assert L.smx_ctx_set_cost(ctx, 3, None) == -1                           # only smx_ctx_set_zncc writes the mode
        assert L.smx_ctx_set_zncc(ctx, C.byref(_zp(5, 3))) == -1 and L.smx_ctx_set_zncc(ctx, C.byref(_zp(3, 0))) == -1
        maps = [k for k in names if not k.startswith(("cost", "agg"))]
        p = smx.default_zncc_params()
        _lib.check(L.smx_ctx_set_zncc(ctx, C.byref(p)))
        assert L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR) == -1
        assert "the ZNCC cost is on (smx_ctx_set_zncc)" in L.smx_last_error().decode()
        for fields in (maps, list(names)):                      # through the chunk buffer, then with the whole volumes
            for k, v in run(fields).items():
                _eq(v, e[names[k]], f"zncc ctx {k}")
        # another window changes the volume
        _lib.check(L.smx_ctx_set_zncc(ctx, C.byref(_zp(1, 4))))
        _eq(run(["cost_l"])["cost_l"], ref.zncc_cost(Il, Ir, D, DMINL, 1, 4), "zncc 3x9 ctx cost_l")
        # and back
        _lib.check(L.smx_ctx_set_zncc(ctx, None))
        for k, v in run(maps + ["cost_l", "cost_r"]).items():
            _eq(v, plain[names[k]], f"reference ctx {k}")
        _lib.check(L.smx_ctx_stereo_pair_async(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR))
        _lib.check(L.smx_ctx_wait(ctx, None, None))
    finally:
        L.smx_destroy(ctx)
