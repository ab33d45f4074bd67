"""The memory contract of the aggregation entries (include/smx.h), on the GPU: guards, poison, minimal workspace.

Every other GPU test compares WHAT the kernels compute.  This one also checks WHERE they write and what they assume about
memory they did not write: each buffer of a call -- workspace, keys, mean, aggregated volume, neighbour state, the two gray
images, the two cost volumes -- lives in its own tests/guarded.py Guarded (front guard | payload | back guard, all filled
with a poison byte), the workspace is the smallest one the layout accepts (the size tests/test_agg_workspace.py bisects
from the same hook) at a pointer 1, 0 or 4 bytes past a 256-byte boundary, and its contents on entry are 0xA5, 0xFF or what
a call of another path and shape left.  The results must be the oracle's, bit for bit, every guard byte must survive and
every input must be unchanged.  One raw C-ABI call per case (PairPipeline sizes its own buffers).

Shapes: the smallest that have every kind of tile of a walker -- (2, 1), one exact strip x band, one more in both directions
(w*h odd: planes are no 8-byte multiples), two strips plus a ragged quarter by two bands plus half -- from smx_agg_geometry
(the literal constants of test_gpu_parity.py, pinned to the library in every test).  D = 5 with labels that leave the image
on both sides.

Run on the GPU box:  python -m pytest tests/test_gpu_memory_contract.py -m gpu -q
"""
import collections
import ctypes as C
import math

import numpy as np
import pytest

import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib

import subpix_ref
from guarded import SMX_E_WS, Guarded, agg_chunk, hooks, min_workspace
from test_gpu_parity import _COMB, _RING, _eq, _geometry

pytestmark = pytest.mark.gpu

D = 5
DMIN = (-2, -3)          # left, right: partners leave the image on both sides
IDENTITY = np.iinfo(np.int64).max

# forced: smx_set_agg_path;  cost: materialised volumes;  agg: the caller's volume (else the walker's own q planes);
# nbr: the _nbr entry;  bad: one -0.75 in the left volume (the queued ring walker reruns);  geom: whose tiles the shapes follow
Case = collections.namedtuple("Case", "forced radius cost agg nbr bad geom")
CASES = {
    "comb-images":          Case(5, 9, False, False, False, False, _COMB),
    "comb-images-agg":      Case(5, 9, False, True, False, False, _COMB),
    "comb-costs-agg":       Case(5, 9, True, True, False, False, _COMB),
    "comb-costs-q":         Case(5, 9, True, False, False, False, _COMB),
    "comb-costs-bad-q":     Case(5, 9, True, False, False, True, _COMB),
    "comb-costs-bad-agg":   Case(5, 9, True, True, False, True, _COMB),
    "ring-r9":              Case(3, 9, False, False, False, False, _RING),
    "ring-r4-costs-agg":    Case(3, 4, True, True, False, False, _RING),
    "ring-r0-agg":          Case(3, 0, False, True, False, False, _RING),
    "multi-r12-auto-agg":   Case(0, 12, False, True, False, False, _RING),
    "multi-r9-forced-costs": Case(1, 9, True, False, False, False, _RING),
    "comb-images-nbr":      Case(5, 9, False, False, True, False, _COMB),
    "comb-costs-nbr":       Case(5, 9, True, False, True, False, _COMB),
    "comb-costs-bad-nbr":   Case(5, 9, True, True, True, True, _COMB),
    "ring-r9-nbr":          Case(3, 9, False, False, True, False, _RING),
    "ring-r4-costs-nbr":    Case(3, 4, True, True, True, False, _RING),
    "fast-r9":              Case(4, 9, False, False, False, False, _COMB),
    "fast-r4-agg":          Case(4, 4, False, True, False, False, _RING),
}


def _shapes(geom):
    ow, bh = geom
    return [(2, 1), (ow, bh), (ow + 1, bh + 1), (2 * ow + ow // 4, 2 * bh + bh // 2)]


assert _shapes(_COMB)[-1] == (342, 25) and _shapes(_RING)[-1] == (144, 40)
assert all((w * h) % 2 for w, h in (_shapes(_COMB)[2], _shapes(_RING)[2]))


@pytest.fixture(scope="module")
def so():
    smx.lib()                    # first: binds the library to torch's HIP runtime (_lib._preload_torch_hip_runtime)
    assert _geometry(9)[:2] == _COMB
    smx.lib().smx_set_agg_path(3)
    try:
        assert _geometry(9)[:2] == _RING and _geometry(4)[:2] == _RING
    finally:
        smx.lib().smx_set_agg_path(0)
    return hooks(_lib.SO_PATH, _lib.Params)


def _params(radius):
    p = smx.default_params()
    p.radius = radius
    return p


def _forced(case, w, h):
    """The comb walker takes materialised volumes from one 16-byte quad per plane on (smx_agg.hip v5_applies): below that
    the case runs as `fused, walker chosen as in auto`, which is the ring walker."""
    return 2 if case.forced == 5 and case.cost and w * h < 4 else case.forced


# ---- inputs and the oracle's answers, computed once per (shape, radius, bad) and left unchanged -----------------------------
_DATA = {}


def _data(orc, w, h, radius, bad):
    key = (w, h, radius, bad)
    if key not in _DATA:
        rng = np.random.default_rng(1000 * w + h)
        base = rng.integers(0, 256, size=(h, w + 16), dtype=np.uint8)
        imgs = [np.ascontiguousarray(base[:, :w]), np.ascontiguousarray(base[:, 2:2 + w])]
        po = orc.Params.from_buffer_copy(bytes(_params(radius)))
        costs = [orc.cost_volume(imgs[0], imgs[1], D, DMIN[0], po), orc.cost_volume(imgs[1], imgs[0], D, DMIN[1], po)]
        if bad:
            costs[0][2, h // 2, w // 2] = np.float32(-0.75)
        views = []
        for v in range(2):
            best, dmap, mean, agg = orc.guided_filter(imgs[v], costs[v], DMIN[v], want_agg=True, params=po)
            keys = orc.pack_keys(best, (dmap - DMIN[v]).astype(np.int64))
            z, c0, lo, hi, last = subpix_ref.winners(agg)
            assert (z >= 0).all() and np.array_equal(keys, orc.pack_keys(c0, z))       # both references name one winner
            views.append(dict(keys=keys, mean=mean, agg=agg, nbr=np.stack([lo, hi, last])))
        for a in imgs + costs + [x for v in views for x in v.values()]:
            a.setflags(write=False)
        _DATA[key] = (imgs, costs, views)
    return _DATA[key]


# ---- one call ----------------------------------------------------------------------------------------------------------------
class Call:
    """One aggregation call through the raw C-ABI with every buffer in its own Guarded.  ws_misalign: the workspace pointer's
    distance from a 256-byte boundary;  fill: the poison of the workspace and of every output;  ws_content: bytes (a CPU uint8
    tensor) the workspace holds on entry instead of `fill`, repeated to its size;  shifted: outputs at the smallest alignment
    of their type past a 256-byte boundary, and keys handed over IN/OUT as the identity instead of declared fresh."""

    def __init__(self, orc, so, case, nviews, w, h, ws_bytes, ws_misalign, fill=0xA5, ws_content=None, shifted=False):
        import torch
        self.case, self.nviews, self.w, self.h = case, nviews, w, h
        n = w * h
        imgs, costs, self.want = _data(orc, w, h, case.radius, case.bad)
        G = lambda dtype, shape, mis=0, f=fill: Guarded(int(np.prod(shape)) * np.dtype(dtype).itemsize, dtype, shape,
                                                        misalign=mis, fill=f, plane=n)
        self.ws = G(np.uint8, (ws_bytes,), ws_misalign)
        if ws_content is not None:
            reps = -(-ws_bytes // ws_content.numel())
            self.ws.bytes.copy_(ws_content.repeat(reps)[:ws_bytes])
        self.keys = G(np.int64, (nviews, h, w), 8 if shifted else 0)
        self.mean = G(np.uint8, (nviews, h, w), 1 if shifted else 0)
        self.agg = G(np.float32, (nviews, D, h, w), 4 if shifted else 0) if case.agg else None
        self.nbr = G(np.float32, (nviews, 3, h, w), 4 if shifted else 0) if case.nbr else None
        self.gray = [G(np.uint8, (h, w)).load(im) for im in imgs]
        self.cost = [G(np.float32, (D, h, w)).load(c) for c in costs[:nviews]] if case.cost else []
        if shifted:
            self.keys.view.fill_(IDENTITY)
        L = smx.lib()
        p = _params(case.radius)
        forced = _forced(case, w, h)
        ptr = lambda g: g.ptr if g is not None else None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        cost = [ptr(c) for c in self.cost] + [None, None]
        out = (ptr(self.keys), ptr(self.mean), ptr(self.agg), self.ws.ptr, ws_bytes)
        L.smx_set_agg_path(forced)
        L.smx_set_keys_fresh(0 if shifted else 1)
        try:
            if nviews == 1:
                args = (C.byref(p), self.gray[0].ptr, self.gray[1].ptr, cost[0], w, h, DMIN[0], 0, D, *out)
                self.rc = (L.smx_dev_aggregate_wta_nbr(*args, self.nbr.ptr, st) if case.nbr else
                           L.smx_dev_aggregate_wta(*args, st))
            else:
                head = (C.byref(p), self.gray[0].ptr, self.gray[1].ptr)
                tail = (w, h, DMIN[0], DMIN[1], 0, D, *out)
                if case.nbr:
                    self.rc = L.smx_dev_aggregate_wta_pair_nbr(*head, cost[0], cost[1], *tail, self.nbr.ptr, st)
                elif case.cost:
                    self.rc = L.smx_dev_aggregate_wta_pair_cost(*head, cost[0], cost[1], *tail, st)
                else:
                    self.rc = L.smx_dev_aggregate_wta_pair(*head, *tail, st)
            self.error = L.smx_last_error().decode() if self.rc else ""
            self.ran = L.smx_last_agg_path()
            c, k = C.c_int(0), C.c_int(0)
            L.smx_last_agg_chunk(C.byref(c), C.byref(k))
            self.chunk = (c.value, k.value)
        finally:
            L.smx_set_agg_path(0)
            L.smx_set_keys_fresh(0)
        torch.cuda.synchronize()

    def outputs(self):
        return [(k, g) for k, g in (("keys", self.keys), ("mean", self.mean), ("agg", self.agg), ("nbr", self.nbr)) if g]

    def results(self):
        return {k: g.numpy() for k, g in self.outputs()}

    def verify(self, so, what, want=None):
        """Status, path and fall-back report; the results (the oracle's, or `want`: the results of another call); then every
        guard and every input.  All findings of the call are reported together."""
        case, nviews, w, h = self.case, self.nviews, self.w, self.h
        assert self.rc == 0, f"{what}: {self.rc} {self.error}"
        L = smx.lib()
        assert L.smx_dev_agg_status(self.ws.ptr) == 0, f"{what}: {L.smx_last_error().decode()}"
        path = C.c_int(0)
        assert so.smx_debug_agg_path(C.byref(_params(case.radius)), w, h, nviews, int(case.cost), _forced(case, w, h),
                                     C.byref(path)) == 0
        assert self.ran == path.value, (what, self.ran, path.value)
        fb = C.c_int(-1)
        assert L.smx_dev_agg_fallback(self.ws.ptr, C.byref(fb)) == 0
        assert fb.value == int(case.bad and self.ran == 5), f"{what}: fall-back report {fb.value}"
        errs = []

        def collect(fn, *a):
            try:
                fn(*a)
            except AssertionError as e:
                errs.append(str(e))

        got = self.results()
        for k in got:
            if want is not None:
                collect(_eq, got[k], want[k], f"{what} {k}")
            else:
                for v in range(nviews):
                    collect(_eq, got[k][v], self.want[v][k], f"{what} view {v} {k}")
        collect(self.ws.check, f"{what} workspace")
        for k, g in self.outputs():
            collect(g.check, f"{what} d_{k}")
        for i, g in enumerate(self.gray):
            collect(g.check_unchanged, f"{what} gray image {i}")
        for i, g in enumerate(self.cost):
            collect(g.check_unchanged, f"{what} cost volume {i}")
        assert not errs, "\n".join(errs)

    def verify_refused(self, what):
        """SMX_E_WS, nothing launched: every guard, every output payload and the workspace still hold the poison."""
        assert self.rc == SMX_E_WS, f"{what}: {self.rc} {self.error}"
        self.ws.check_untouched(f"{what} workspace")
        for k, g in self.outputs():
            g.check_untouched(f"{what} d_{k}")
        for g in self.gray + self.cost:
            g.check_unchanged(f"{what} input")


def _min_ws(so, case, nviews, w, h, n):
    """The smallest workspace of the call, with what tests/test_agg_workspace.py asserts of the same bisection: it holds, one
    256-byte step below it the call is refused, and it is within the documented size and not below the planes every call
    writes (fused) / exactly the ten planes of the multi-kernel path."""
    p, forced = _params(case.radius), _forced(case, w, h)
    args = (p, w, h, nviews, int(case.cost), int(not case.agg), forced)
    ws = min_workspace(so, *args, n)
    got, rc = agg_chunk(so, *args, ws, n)
    assert rc == 0 and got >= 1
    assert agg_chunk(so, *args, ws - 256, n) == (None, SMX_E_WS)
    assert ws <= nviews * so.smx_agg_workspace_bytes(w, h, 1)
    path = C.c_int(0)
    assert so.smx_debug_agg_path(C.byref(p), w, h, nviews, int(case.cost), forced, C.byref(path)) == 0
    if path.value == 1:
        assert ws == 512 + 10 * ((4 * w * h + 255) // 256 * 256)
    else:
        assert ws >= 256 + 2 * (w + 8) * h * 4 + nviews * w * h * (16 + (0 if case.agg else 4))
    if forced in (2, 4, 5):
        # (the host test bisects auto mode and the forced ring walker: a forced path that runs auto mode's walker has its size)
        assert ws == min_workspace(so, *args[:-1], 0, n)
    return ws, got


# FAST is not bit-exact: its reference is the same call in a roomy workspace of zeros (independence from the workspace, not
# correctness, is the property here)
_FAST = {}


def _want(orc, so, name, nviews, w, h):
    case = CASES[name]
    if case.forced != 4:
        return None
    key = (name, nviews, w, h)
    if key not in _FAST:
        roomy = nviews * so.smx_agg_workspace_bytes(w, h, D)
        c = Call(orc, so, case, nviews, w, h, roomy, 0, fill=0)
        assert c.rc == 0 and c.ran == 4 and c.chunk == (D, 1), (c.rc, c.error, c.ran, c.chunk)
        _FAST[key] = c.results()
    return _FAST[key]


_RUNS = [(name, w, h) for name, case in CASES.items() for (w, h) in _shapes(case.geom)]


@pytest.mark.parametrize("nviews", [1, 2])
@pytest.mark.parametrize("name,w,h", _RUNS, ids=[f"{n}-{w}x{h}" for n, w, h in _RUNS])
def test_minimal_workspace(orc, so, name, w, h, nviews):
    """(a) the smallest workspace for the call's five slices at a pointer 1 byte past a 256-byte boundary -- the 255 lost
    bytes the bisection assumes; (b) the same size on the boundary, outputs at the smallest alignment of their types and keys
    IN/OUT, and 4 bytes past it for the fused walkers; (c) the smallest workspace for ONE slice with five slices to do: the
    launches the layout says, one slice each wherever a slice's planes exceed the 256-byte step; (d) one step below (a):
    SMX_E_WS and nothing written."""
    case = CASES[name]
    want = _want(orc, so, name, nviews, w, h)
    ws, _ = _min_ws(so, case, nviews, w, h, D)
    fused = None
    for tag, mis, shifted in (("(a) misalign 1", 1, False), ("(b) misalign 0", 0, True), ("(b) misalign 4", 4, True)):
        if mis == 4 and fused is False:
            continue
        c = Call(orc, so, case, nviews, w, h, ws, mis, shifted=shifted)
        c.verify(so, f"{name} {w}x{h} nviews={nviews} {tag}", want)
        fused = c.ran != 1
    ws1, chunk = _min_ws(so, case, nviews, w, h, 1)
    c = Call(orc, so, case, nviews, w, h, ws1, 1)
    c.verify(so, f"{name} {w}x{h} nviews={nviews} (c) one slice", want)
    chunk, rc = agg_chunk(so, _params(case.radius), w, h, nviews, int(case.cost), int(not case.agg), _forced(case, w, h), ws1, D)
    assert rc == 0 and (chunk == 1 or (w, h) == (2, 1)), chunk
    if fused:
        assert c.chunk == (chunk, math.ceil(D / chunk)), (c.chunk, chunk)
        assert (w, h) == (2, 1) or c.chunk == (1, 5)
    c = Call(orc, so, case, nviews, w, h, ws - 256, 1)
    c.verify_refused(f"{name} {w}x{h} nviews={nviews} (d) one step below")


# ---- what the workspace holds on entry -------------------------------------------------------------------------------------
# the largest shape of each case (every kind of tile), and the ring walker at radius 4 on 129 x 33 behind the comb walker
_POISON = [(name, *_shapes(case.geom)[-1]) for name, case in CASES.items()] + [("ring-r4-costs-agg", 129, 33)]
_LEFT = {}


def _leftover(orc, so, name, nviews, w, h):
    """The workspace bytes a call of another path and shape leaves behind: the ring walker at radius 4 on 129 x 33 for the
    comb walker's cases, the comb walker on 342 x 25 for every other."""
    other = ("ring-r4-costs-agg", 129, 33) if CASES[name].geom == _COMB else ("comb-images", 342, 25)
    key = other + (nviews,)
    if key not in _LEFT:
        oc = CASES[other[0]]
        ws, _ = _min_ws(so, oc, nviews, other[1], other[2], D)
        c = Call(orc, so, oc, nviews, other[1], other[2], ws, 1)
        c.verify(so, f"leftover source {other}")
        _LEFT[key] = c.ws.bytes.cpu()
    return _LEFT[key]


@pytest.mark.parametrize("nviews", [1, 2])
@pytest.mark.parametrize("name,w,h", _POISON, ids=[f"{n}-{w}x{h}" for n, w, h in _POISON])
def test_workspace_contents_do_not_matter(orc, so, name, w, h, nviews):
    """The minimal workspace of (a) holding, in this order, what a call of another path and shape left in it, 0xA5
    everywhere, 0xFF everywhere (NaN floats, tickets and flags of -1, every status word set): the same results, status OK,
    the fall-back report of this call alone.  Outputs carry the same poison."""
    case = CASES[name]
    want = _want(orc, so, name, nviews, w, h)
    ws, _ = _min_ws(so, case, nviews, w, h, D)
    left = _leftover(orc, so, name, nviews, w, h)
    for tag, fill, content in (("leftover", 0xA5, left), ("0xA5", 0xA5, None), ("0xFF", 0xFF, None)):
        c = Call(orc, so, case, nviews, w, h, ws, 1, fill=fill, ws_content=content)
        c.verify(so, f"{name} {w}x{h} nviews={nviews} workspace {tag}", want)
