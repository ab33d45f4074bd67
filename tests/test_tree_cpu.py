"""The non-local tree filter without a GPU (include/smx.h, above smx_tree_params; tests/tree_ref.py):
  the reference   the two sweeps against the brute force out[p] = sum_q exp(-dist_tree(p, q) / sigma) C[q] in float64 with the
                  distances from an all-pairs walk of the tree, on 7 x 5 and 12 x 1; the vectorised form against the node-by-node
                  one, bit for bit
  the tree        a spanning tree of minimum total weight (an independent Prim in this module gives the same total), the comb
                  on a constant image -- all ties fall to the id order --, single rows, columns and pixels
  the library     smx_tree_build's blob byte for byte, the tables, the defaults and the sizes of the built library (host-only
                  entries: no device call), and the same host code as a stand-alone program under the sanitizers
                  (tests/host_tree_check.cpp)
  the scene       what the method buys and what it does not: the band scene of tests/test_perm_cpu.py under guide noise

The scene, in figures.  192 x 48, random texture with a band of 60 columns at gray 128 (left columns 60 .. 119, true label -6),
gaussian noise of sigma 1 everywhere and, IN THE BAND, uniform noise of amplitude A, independent in the two images.  Wrong exact
labels among the 8256 kept pixels (columns 20 ..: those whose match lies inside the right image) of the winner-take-all left map,
the guided filter's volume behind the permeability filter at sigma 8 / 16 / 32 / 64 / 128 and behind the tree filter at its
default sigma 25.5, never tuned:
    A  seed   guided filter   permeability 8 / 16 / 32 / 64 / 128      tree 25.5
    2   0        1429            975 /   99 /   0 /  0 / 0                  0
    2   1        1418            935 /   99 /   0 /  0 / 0                  0
    4   0        1450           1263 /  830 /   0 /  0 / 0                394
    4   1        1550           1366 / 1012 /  67 /  0 / 0                511
    8   0        1471           1370 / 1225 / 783 /  0 / 0                958
    8   1        1574           1482 / 1328 / 968 / 50 / 0                971
(and at A = 12, 16, 24 the same picture: permeability at sigma 128 stays at 0 or 1, the tree filter at 1158 .. 1453).  The
condition aimed for -- the tree filter wrong on at most 1 % of the kept pixels where permeability at its best sigma is
wrong on ten times as many -- holds at NO amplitude of this family, and the margin is NOT claimed: the band is bounded by hard
texture, whose steps of ~85 gray levels stop the permeability pass at any sigma, so its best sigma simply grows with the noise,
while the tree's paths through the band are long (its edges are the band's smallest, its paths are tortuous) and pay every step
at the fixed sigma.  What the tree filter does show here: at its one default sigma it repairs the band exactly up to A = 2, where
permeability needs sigma >= 32.  The test asserts these counts and nothing more.

Run anywhere:  python -m pytest tests -q -m "not gpu" -k tree_cpu
"""
import ctypes as C
import heapq
import os
import shutil
import subprocess

import numpy as np
import pytest

import perm_ref
import tree_ref as ref
from test_host_twins_cpu import BUILDS, ROOT

F32 = np.float32
CSRC = os.path.join(ROOT, "stereo_matching_cuda_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _guide(rng, h, w, ch, kind):
    if kind == "random":
        g = rng.integers(0, 256, (h, w, ch))
    elif kind == "two":
        g = rng.integers(0, 2, (h, w, ch)) * 9 + 100
    elif kind == "extreme":
        g = rng.integers(0, 2, (h, w, ch)) * 255
    else:
        g = np.full((h, w, ch), 77)
    g = g.astype(np.uint8)
    return g[:, :, 0] if ch == 1 else g


# ---------------------------------------------------------------------------------------------
# the reference against the brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(5, 7), (1, 12)])
@pytest.mark.parametrize("kind", ["random", "two"])
def test_the_two_sweeps_equal_the_sum_over_tree_distances(h, w, kind):
    """Relative 1e-5: the costs are positive, so nothing cancels, and f32 rounding of at most 35 terms with two operations a term
    stays below 2 * 35 * 2^-24 = 4.2e-6 (derived, not measured)."""
    rng = np.random.default_rng(h * 100 + w)
    for ch, sigma in ((1, ref.DEFAULT_SIGMA), (3, 7.0), (4, 90.0)):
        g = _guide(rng, h, w, ch, kind)
        vol = rng.uniform(0.5, 1.5, (3, h, w)).astype(F32)
        tree = ref.build(g)
        dist = ref.tree_distances(tree)
        want = (np.exp(-dist / sigma) @ vol.reshape(3, -1).astype(np.float64).T).T.reshape(3, h, w)
        got = ref.filter_volume(vol, g, sigma, tree)
        assert np.max(np.abs(got - want) / want) <= 1e-5
        assert np.array_equal(bits(got), bits(ref.filter_volume_loops(vol, g, sigma)))


def test_nan_and_inf_stay_in_their_slice():
    rng = np.random.default_rng(2)
    g = _guide(rng, 5, 7, 1, "random")
    vol = rng.standard_normal((4, 5, 7)).astype(F32)
    clean = ref.filter_volume(vol, g)
    vol[1, 2, 3], vol[2, 0, 0] = np.nan, np.inf
    out = ref.filter_volume(vol, g)
    assert np.isnan(out[1]).all() and not np.isfinite(out[2]).any()
    assert np.array_equal(bits(out[[0, 3]]), bits(clean[[0, 3]]))
    a, b = bits(out), bits(ref.filter_volume_loops(vol, g))
    assert ((a == b) | (np.isnan(out) & np.isnan(b.view(F32)))).all()


# ---------------------------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------------------------
def _prim_total(g):
    """the total weight of a minimum spanning tree of the 4-grid of g by Prim's algorithm with a heap: another algorithm, its own
    weights"""
    g = g.astype(np.int64)
    if g.ndim == 2:
        g = g[:, :, None]
    h, w = g.shape[:2]

    def weight(a, b):
        return int(np.abs(g[a] - g[b])[:3].max())

    seen = np.zeros((h, w), bool)
    heap, total, count = [(0, 0, 0)], 0, 0
    while heap:
        k, y, x = heapq.heappop(heap)
        if seen[y, x]:
            continue
        seen[y, x] = True
        total += k
        count += 1
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < h and 0 <= xx < w and not seen[yy, xx]:
                heapq.heappush(heap, (weight((y, x), (yy, xx)), yy, xx))
    assert count == h * w
    return total


def _check_structure(tree, g):
    """a spanning tree of the 4-grid in breadth-first order with the weights of the guide"""
    n, h, w = tree["n"], tree["h"], tree["w"]
    order, parent, cf, cc, wt, ls = (tree[k].astype(np.int64) for k in ("order", "parent", "child_first", "child_count", "wt", "level_start"))
    assert sorted(order.tolist()) == list(range(n)) and order[0] == 0 and parent[0] == 0 and wt[0] == 0
    assert ls[0] == 0 and ls[-1] == n and (np.diff(ls) > 0).all() and len(ls) == tree["levels"] + 1
    level = np.repeat(np.arange(tree["levels"]), np.diff(ls))
    gg = g.astype(np.int64).reshape(n, -1)[:, :3]
    for i in range(1, n):
        p, q = order[i], order[parent[i]]
        assert abs(p - q) in (1, w) and (abs(p - q) == w or p // w == q // w)      # 4-neighbours
        assert wt[i] == np.abs(gg[p] - gg[q]).max()
        assert level[i] == level[parent[i]] + 1
        assert cf[parent[i]] <= i < cf[parent[i]] + cc[parent[i]]
    assert cc.sum() == n - 1 and (np.diff(cf) >= 0).all()
    for i in range(n):                                                              # children in ascending pixel index
        kids = order[cf[i]:cf[i] + cc[i]]
        assert (np.diff(kids) > 0).all()


@pytest.mark.parametrize("h,w,ch,kind", [(5, 7, 1, "random"), (9, 4, 3, "random"), (6, 6, 4, "two"), (8, 5, 1, "extreme"), (1, 12, 1, "random"),
                                         (12, 1, 3, "two"), (1, 1, 1, "random"), (2, 2, 1, "random"), (23, 31, 1, "two"), (23, 31, 3, "random")])
def test_the_tree_is_a_minimum_spanning_tree_in_breadth_first_order(h, w, ch, kind):
    rng = np.random.default_rng(h * 1000 + w * 10 + ch)
    g = _guide(rng, h, w, ch, kind)
    tree = ref.build(g)
    _check_structure(tree, g)
    assert int(tree["wt"].astype(np.int64).sum()) == _prim_total(g)


def test_a_constant_image_gives_the_comb_and_the_plain_sum():
    """every weight is 0, so the edges join in id order: edge 2p (right) before 2p + 1 (down) for p ascending.  Along row 0 every
    right edge joins; every down edge joins (its lower pixel is still alone when its turn comes, all ids of row y lie before
    those of row y + 1); a right edge of a row below the first finds both ends hanging from row 0 already.  The comb: the top
    row and every vertical edge."""
    h, w = 6, 9
    g = np.full((h, w), 200, np.uint8)
    tree = ref.build(g)
    order, parent = tree["order"].astype(np.int64), tree["parent"].astype(np.int64)
    for i in range(1, h * w):
        p, q = order[i], order[parent[i]]
        assert q == (p - 1 if p < w else p - w)
    assert tree["levels"] == w + h - 1 and (tree["wt"] == 0).all()
    rng = np.random.default_rng(0)
    vol = rng.integers(-8, 9, (3, h, w)).astype(F32)            # (small integers: every sum is exact in any order)
    out = ref.filter_volume(vol, g, 3.0)
    assert np.array_equal(out, np.broadcast_to(vol.sum(axis=(1, 2))[:, None, None], out.shape))


def test_single_pixel_row_and_column():
    rng = np.random.default_rng(4)
    one = rng.standard_normal((3, 1, 1)).astype(F32)
    assert np.array_equal(bits(ref.filter_volume(one, np.zeros((1, 1), np.uint8))), bits(one))
    for h, w in ((1, 6), (6, 1)):
        g = rng.integers(0, 256, (h, w)).astype(np.uint8)
        tree = ref.build(g)
        assert tree["levels"] == h * w and tree["order"].tolist() == list(range(h * w))         # a path
        vol = rng.standard_normal((2, h, w)).astype(F32)
        assert np.array_equal(bits(ref.filter_volume(vol, g, 9.0)), bits(ref.filter_volume_loops(vol, g, 9.0)))


# ---------------------------------------------------------------------------------------------
# the library's host entries (no device call) and the same code under the sanitizers
# ---------------------------------------------------------------------------------------------
BLOBS = [(1, 1, 1, "random"), (1, 12, 1, "random"), (12, 1, 3, "two"), (2, 2, 4, "random"), (5, 7, 1, "random"), (9, 65, 1, "two"),
         (70, 129, 3, "random"), (40, 19, 1, "extreme"), (33, 33, 1, "constant")]
SIGMAS = [25.5, 8.0, 0.001, 0.012, 7.3, 1e6]


def test_the_library_builds_the_same_blob_byte_for_byte():
    import stereo_matching_cuda_amd as smx
    L = smx.lib()
    rng = np.random.default_rng(11)
    for h, w, ch, kind in BLOBS:
        g = _guide(rng, h, w, ch, kind)
        want = ref.blob(ref.build(g))
        assert L.smx_tree_bytes(w, h) == want.size == ref.tree_bytes(w, h)
        got = smx.tree_build(g)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (h, w, ch, kind)
    for bad in ((0, 4), (4, 0), (1 << 16, 1 << 15)):
        assert L.smx_tree_bytes(*bad) == 0
    buf = np.zeros(64, np.uint32)
    g = np.zeros((2, 2), np.uint8)
    for args in ((g.ctypes.data, 2, 2, 2, buf.ctypes.data), (g.ctypes.data, 1, 0, 2, buf.ctypes.data), (None, 1, 2, 2, buf.ctypes.data),
                 (g.ctypes.data, 1, 2, 2, None), (g.ctypes.data, 1, 2, 2, buf.ctypes.data + 1)):
        assert L.smx_tree_build(*args) == -1 and L.smx_last_error()
    assert not buf.any()


def test_tables_defaults_and_sizes_of_the_library():
    import stereo_matching_cuda_amd as smx
    L = smx.lib()
    assert smx.default_tree_params().sigma == 25.5 == ref.DEFAULT_SIGMA
    for sigma in SIGMAS:
        p = smx.default_tree_params()
        p.sigma = sigma
        t, u = smx.tree_tables(p)
        wt, wu = ref.tables(sigma)
        assert np.array_equal(bits(np.array(t, F32)), bits(wt)) and np.array_equal(bits(np.array(u, F32)), bits(wu))
        assert t[0] == 1.0 and u[0] == 0.0
    t = (C.c_float * 256)()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        p = smx.default_tree_params()
        p.sigma = bad
        assert L.smx_tree_tables(C.byref(p), t, t) == -1 and b"sigma" in L.smx_last_error()
        with pytest.raises(ValueError):
            smx.tree_filter(np.zeros((1, 2, 2), F32), np.zeros((2, 2), np.uint8), bad)
    with pytest.raises(ValueError):
        smx.tree_filter(np.zeros((1, 2, 2), F32), np.zeros((3, 2), np.uint8))
    assert L.smx_tree_workspace_bytes(19, 40, 17, 2) == 2 * 19 * 40 * 4 * 2 * 17
    for bad in ((0, 4, 1, 1), (4, 0, 1, 1), (4, 4, 0, 1), (4, 4, 1, 0), (4, 4, 1, 3), (1 << 16, 1 << 15, 1, 1)):
        assert L.smx_tree_workspace_bytes(*bad) == 0


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_host_code_equals_the_reference_as_a_stand_alone_program(build, tmp_path):
    """Exit status 0, a clean stderr (the sanitised build is the program itself, nothing preloaded), every blob and table equal
    to the reference's."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "host_tree_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[build] +
                          ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(ROOT, "tests", "host_tree_check.cpp"), "-o", exe])
    work = tmp_path / "cases"
    work.mkdir()
    rng = np.random.default_rng(12)
    lines, checks = [], []
    for k, (h, w, ch, kind) in enumerate(BLOBS):
        g = _guide(rng, h, w, ch, kind)
        g.tofile(work / f"b{k}.guide.u8")
        lines.append(f"build b{k} {w} {h} {ch}")
        checks.append((f"b{k}.blob.u8", np.uint8, ref.blob(ref.build(g))))
    for k, sigma in enumerate(SIGMAS):
        lines.append(f"tables t{k} {sigma!r}")
        t, u = ref.tables(sigma)
        checks += [(f"t{k}.t.f32", "<f4", t), (f"t{k}.u.f32", "<f4", u)]
    (work / "cases.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    assert f"cases {len(lines)}\n" in r.stdout
    for name, dt, want in checks:
        got = np.fromfile(work / name, dt)
        assert got.size == want.size and np.array_equal(got.view(np.uint8), want.view(np.uint8)), name


# ---------------------------------------------------------------------------------------------
# what the method buys, and what it does not (the module's docstring has the table)
# ---------------------------------------------------------------------------------------------
W, H, D, DMINL, DMINR = 192, 48, 16, -15, 0
SHIFT, BAND = 6, 60
PERM_SIGMAS = (8.0, 16.0, 32.0, 64.0, 128.0)
# (amplitude, seed) -> (guided filter, permeability at PERM_SIGMAS, tree at its default sigma): wrong among the 8256 kept pixels
COUNTS = {(2, 0): (1429, (975, 99, 0, 0, 0), 0), (2, 1): (1418, (935, 99, 0, 0, 0), 0),
          (4, 0): (1450, (1263, 830, 0, 0, 0), 394), (4, 1): (1550, (1366, 1012, 67, 0, 0), 511),
          (8, 0): (1471, (1370, 1225, 783, 0, 0), 958), (8, 1): (1574, (1482, 1328, 968, 50, 0), 971)}


def noisy_band_scene(seed, amp):
    """the band scene of tests/test_perm_cpu.py (the same draws in the same order), then uniform noise of amplitude amp in the
    band of each image, independent in the two"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H, 224)).astype(np.float64)
    base[:, 76:76 + BAND] = 128
    L = base[:, 16:208] + rng.normal(0, 1, (H, W))
    R = base[:, 16 + SHIFT:208 + SHIFT] + rng.normal(0, 1, (H, W))
    L[:, 60:60 + BAND] += rng.uniform(-amp, amp, (H, BAND))
    R[:, 60 - SHIFT:60 - SHIFT + BAND] += rng.uniform(-amp, amp, (H, BAND))
    return tuple(np.clip(np.rint(v), 0, 255).astype(np.uint8) for v in (L, R))


def _wrong(vol):
    m = perm_ref.label_map(perm_ref.winners(vol)[0], DMINL)
    return int((m[:, 20:] + SHIFT != 0).sum())


@pytest.mark.parametrize("amp,seed", sorted(COUNTS))
def test_the_band_under_guide_noise(amp, seed):
    import oracle
    L, R = noisy_band_scene(seed, amp)
    agg = oracle.stereo_pair(L, R, D, dminl=DMINL, dminr=DMINR, want_agg=True)["aggl"]
    got = (_wrong(agg), tuple(_wrong(perm_ref.filter_volume(agg, L, s)) for s in PERM_SIGMAS), _wrong(ref.filter_volume(agg, L)))
    kept = H * (W - 20)
    print(f"amplitude {amp} seed {seed}: wrong of {kept}: guided filter {got[0]}, permeability {got[1]} at {PERM_SIGMAS}, tree {got[2]}")
    assert kept == 8256 and got == COUNTS[(amp, seed)]
    # what is claimed: the tree filter at its one sigma repairs the band up to amplitude 2; NOT claimed: any margin over
    # permeability at its best sigma, which stays exact at every amplitude here
    assert min(got[1]) == 0 and (got[2] == 0) == (amp <= 2)
