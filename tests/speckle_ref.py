"""Plain numpy reference of the speckle filter of include/smx.h (smx_speckle_filter): which pixels count, which
4-neighbours are joined, the connected components of that graph, and the rewrite of the small ones.

A helper module (imported by name; no fixtures).  The edge lists are built with array operations and the components come
from a small vectorised union-find: every edge hooks the larger of its two roots under the smaller one (np.minimum.at),
then every pixel is pointed at its root, until no edge joins two roots.  The label of a component is therefore its
smallest linear index -- the label the GPU forest ends with.  No scipy.
"""
import numpy as np


def counts(disp, vmin):
    """p counts iff disp[p] is finite and (float)(int)disp[p] >= vmin: fill_occlusion's validity test, the conversion
    truncating toward zero and saturating at +-2^31."""
    d = np.ascontiguousarray(disp, np.float32)
    finite = np.isfinite(d)
    t = np.clip(np.trunc(np.where(finite, d, np.float32(0))), np.float32(-2147483648.0), np.float32(2147483648.0))
    return finite & (t.astype(np.float32) >= np.float32(vmin))


def edges(disp, vmin, max_diff):
    """(a, b): linear indices of the joined 4-neighbour pairs, a < b (right neighbours first, then lower ones)."""
    d = np.ascontiguousarray(disp, np.float32)
    h, w = d.shape
    c = counts(d, vmin)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    md = np.float32(max_diff)
    with np.errstate(invalid="ignore", over="ignore"):
        jr = c[:, :-1] & c[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= md)
        jd = c[:-1, :] & c[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= md)
    a = np.concatenate([idx[:, :-1][jr], idx[:-1, :][jd]])
    b = np.concatenate([idx[:, 1:][jr], idx[1:, :][jd]])
    return a, b


def _flatten(parent):
    while True:
        pp = parent[parent]
        if np.array_equal(pp, parent):
            return parent
        parent = pp


def components(disp, vmin, max_diff):
    """(label, size): label[p] = the smallest linear index of p's component, -1 where p does not count; size[p] = the
    number of pixels of p's component, 0 where p does not count.  Both (h, w) int64."""
    d = np.ascontiguousarray(disp, np.float32)
    h, w = d.shape
    a, b = edges(d, vmin, max_diff)
    parent = np.arange(h * w, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        open_ = ra != rb
        if not open_.any():
            break
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        parent = _flatten(parent)
    c = counts(d, vmin).ravel()
    label = np.where(c, parent, -1)
    per_root = np.bincount(parent[c], minlength=h * w)
    size = np.where(c, per_root[parent], 0)
    return label.reshape(h, w), size.reshape(h, w)


def speckle_filter(disp, vmin, new_val, max_size=200, max_diff=1.0):
    """out[p] = new_val iff p counts and its component has <= max_size pixels; every other pixel bit for bit."""
    d = np.ascontiguousarray(disp, np.float32)
    _, size = components(d, vmin, max_diff)
    out = d.copy()
    out[(size > 0) & (size <= int(max_size))] = np.float32(new_val)
    return out


# ---------------------------------------------------------------------------------------------
# maps with long thin components, for the tests
# ---------------------------------------------------------------------------------------------
def spiral(h, w):
    """A one-pixel-wide arm of 1 that winds inwards from (0, 0) with a one-pixel gap of 0 between its turns."""
    s = np.zeros((h, w), np.float32)
    y = x = 0
    dy, dx = 0, 1
    s[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        ahead = 0 <= ay < h and 0 <= ax < w and s[ay, ax] == 1
        if 0 <= ny < h and 0 <= nx < w and s[ny, nx] == 0 and not ahead:
            y, x = ny, nx
            s[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return s


def comb(h, w, vertical=True):
    """A spine along the first row (column) with a tooth on every other column (row), 1 on a background of 0."""
    s = np.zeros((h, w), np.float32)
    if vertical:
        s[0, :] = 1
        s[:, ::2] = 1
    else:
        s[:, 0] = 1
        s[::2, :] = 1
    return s


def structured(h, w):
    """name -> (map, [(max_diff, the size of the largest component at that max_diff, or None where it is not stated)]):
    the maps that stress connectivity, shared by tests/test_gpu_speckle.py and tests/test_host_twins_cpu.py.  With
    vmin 0 every pixel counts.  The ramps a, a + 1, a + 2, ... are one component at max_diff 1 and one per column (row)
    at max_diff 0; the chain 4 5 6 9 joins three columns of every four."""
    y, x = np.mgrid[0:h, 0:w]
    board = ((x + y) % 2).astype(np.float32)
    ramp_x, ramp_y = x.astype(np.float32), y.astype(np.float32)
    return {
        "constant": (np.full((h, w), 3, np.float32), [(0, h * w)]),
        "checkerboard": (board, [(0, 1), (1, h * w)]),
        "spiral": (spiral(h, w), [(0, None)]),
        "comb down": (comb(h, w, True), [(0, None)]),
        "comb right": (comb(h, w, False), [(0, None)]),
        "ramp x": (ramp_x, [(1, h * w), (0, h)]),
        "ramp y": (ramp_y, [(1, h * w), (0, w)]),
        "chain": (np.tile(np.array([4, 5, 6, 9], np.float32), (h, w // 4)), [(1, 3 * h), (0, h)]),
    }
