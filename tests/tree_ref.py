"""numpy reference of the non-local tree filter (include/smx.h, above smx_tree_params; Yang, CVPR 2012): the two weight
tables, the minimum spanning tree of a guide with its breadth-first numbering and blob, the two sweeps of a volume and its
winners.  Nothing is imported from the library; float32 throughout, every product and every sum rounded on its own, so the
kernels' results equal these bit for bit.
"""
import math

import numpy as np

from perm_ref import label_map, pack_keys, winners  # noqa: F401  (the natural-order winner-take-all rule is the same one)

F32 = np.float32
DEFAULT_SIGMA = 25.5


def tables(sigma):
    """(t, u): t[k] = (float)exp(-k / sigma), u[k] = (float)(1 - exp(-2 k / sigma)), k = 0 .. 255, in double (math.exp is the C
    library's exp, as in the library's host code)"""
    t = np.array([math.exp(-float(k) / float(sigma)) for k in range(256)], np.float64).astype(F32)
    u = np.array([1.0 - math.exp(-2.0 * float(k) / float(sigma)) for k in range(256)], np.float64).astype(F32)
    return t, u


def _diff(a, b):
    """|a - b| per pixel: one channel as it is, 3 or 4 channels the maximum over R, G, B (alpha is ignored)"""
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    return d if d.ndim == 2 else d[:, :, :3].max(axis=2)


def edges(guide):
    """-> (ids, weights, h, w) of every edge of the 4-grid: id 2p joins p and p + 1, id 2p + 1 joins p and p + w"""
    g = np.asarray(guide)
    assert g.dtype == np.uint8 and g.ndim in (2, 3)
    if g.ndim == 3 and g.shape[2] == 1:
        g = g[:, :, 0]
    h, w = g.shape[:2]
    p = np.arange(h * w, dtype=np.int64).reshape(h, w)
    ids = np.concatenate([2 * p[:, :-1].ravel(), 2 * p[:-1].ravel() + 1])
    wts = np.concatenate([_diff(g[:, :-1], g[:, 1:]).ravel(), _diff(g[:-1], g[1:]).ravel()])
    return ids, wts.astype(np.int64), h, w


def build(guide):
    """the tree of the guide: Kruskal over the edges in ascending (weight, id) order, pixel 0 the root, the nodes numbered
    breadth first with a node's children in ascending pixel index.  -> dict(n, levels, order, parent, child_first, child_count,
    wt, level_start (levels + 1 entries), h, w)"""
    ids, wts, h, w = edges(guide)
    n = h * w
    up = list(range(n))

    def find(a):
        while up[a] != a:
            up[a] = up[up[a]]
            a = up[a]
        return a

    nbrs = [[] for _ in range(n)]           # (pixel, weight) of the tree's edges at each pixel
    taken = 0
    for k in np.lexsort((ids, wts)):
        e, p = int(ids[k]), int(ids[k]) >> 1
        q = p + (w if e & 1 else 1)
        a, b = find(p), find(q)
        if a == b:
            continue
        up[max(a, b)] = min(a, b)
        nbrs[p].append((q, int(wts[k])))
        nbrs[q].append((p, int(wts[k])))
        taken += 1
    assert taken == n - 1
    order, parent, wt, child_first, child_count, level_start = [0], [0], [0], [], [], [0, 1]
    i = 0
    while True:
        for i in range(i, level_start[-1]):
            p = order[i]
            par = order[parent[i]] if i else -1
            child_first.append(len(order))
            kids = sorted((q, k) for q, k in nbrs[p] if q != par)
            for q, k in kids:
                order.append(q)
                parent.append(i)
                wt.append(k)
            child_count.append(len(kids))
        i = level_start[-1]
        if len(order) == level_start[-1]:
            break
        level_start.append(len(order))
    return dict(n=n, levels=len(level_start) - 1, order=np.array(order, np.uint32), parent=np.array(parent, np.uint32),
                child_first=np.array(child_first, np.uint32), child_count=np.array(child_count, np.uint8),
                wt=np.array(wt, np.uint8), level_start=np.array(level_start, np.uint32), h=h, w=w)


def tree_bytes(w, h):
    return (12 + 18 * w * h + 3) & ~3


def blob(tree):
    """the tree as the library's blob (include/smx.h has the layout): uint8 array of tree_bytes(w, h) bytes"""
    n = tree["n"]
    out = np.zeros(tree_bytes(tree["w"], tree["h"]), np.uint8)
    u32 = out[:12 + 16 * n].view(np.uint32)
    u32[0], u32[1] = n, tree["levels"]
    u32[2:2 + n] = tree["order"]
    u32[2 + n:2 + 2 * n] = tree["parent"]
    u32[2 + 2 * n:2 + 3 * n] = tree["child_first"]
    u32[2 + 3 * n:2 + 3 * n + tree["levels"] + 1] = tree["level_start"]
    out[12 + 16 * n:12 + 17 * n] = tree["child_count"]
    out[12 + 17 * n:12 + 18 * n] = tree["wt"]
    return out


def filter_volume(vol, guide, sigma=DEFAULT_SIGMA, tree=None):
    """vol float32 (D, h, w) -> out (D, h, w): the up sweep and the down sweep of the definition, level by level, every slice at
    once"""
    c = np.ascontiguousarray(vol, F32)
    assert c.ndim == 3
    tr = build(guide) if tree is None else tree
    D, h, w = c.shape
    assert (tr["h"], tr["w"]) == (h, w)
    t, u = tables(sigma)
    order = tr["order"].astype(np.int64)
    cf, cc, wt, par, ls = (tr[k].astype(np.int64) for k in ("child_first", "child_count", "wt", "parent", "level_start"))
    flat = c.reshape(D, -1)
    U = np.empty_like(flat)
    with np.errstate(all="ignore"):
        for lv in range(tr["levels"] - 1, -1, -1):
            i = np.arange(ls[lv], ls[lv + 1])
            U[:, i] = flat[:, order[i]]
            for k in range(4):
                m = i[cc[i] > k]
                ch = cf[m] + k
                U[:, m] = U[:, m] + (t[wt[ch]][None] * U[:, ch]).astype(F32)
        A = U.copy()
        for lv in range(1, tr["levels"]):
            i = np.arange(ls[lv], ls[lv + 1])
            A[:, i] = (t[wt[i]][None] * A[:, par[i]]).astype(F32) + (u[wt[i]][None] * U[:, i]).astype(F32)
    out = np.empty_like(flat)
    out[:, order] = A
    return out.reshape(D, h, w)


def filter_volume_loops(vol, guide, sigma=DEFAULT_SIGMA):
    """the same definition node by node on Python scalars of float32 (for small shapes)"""
    c = np.asarray(vol, F32)
    D, h, w = c.shape
    tr = build(guide)
    t, u = tables(sigma)
    n, order, par, cf, cc, wt = tr["n"], tr["order"], tr["parent"], tr["child_first"], tr["child_count"], tr["wt"]
    out = np.empty((D, n), F32)
    with np.errstate(all="ignore"):
        for z in range(D):
            C = c[z].ravel()
            U = [None] * n
            for i in range(n - 1, -1, -1):          # (any order with the children before their parent)
                s = C[order[i]]
                for k in range(int(cf[i]), int(cf[i]) + int(cc[i])):
                    s = F32(s + F32(t[wt[k]] * U[k]))
                U[i] = s
            A = [None] * n
            A[0] = U[0]
            for i in range(1, n):
                A[i] = F32(F32(t[wt[i]] * A[par[i]]) + F32(u[wt[i]] * U[i]))
            for i in range(n):
                out[z, order[i]] = A[i]
    return out.reshape(D, h, w)


def tree_distances(tree, weights=None):
    """all-pairs distances along the tree (n, n) int64, by a walk from every node (for small shapes)"""
    n, par, wt, order = tree["n"], tree["parent"].astype(np.int64), tree["wt"].astype(np.int64), tree["order"].astype(np.int64)
    adj = [[] for _ in range(n)]
    for i in range(1, n):
        adj[i].append((int(par[i]), int(wt[i])))
        adj[int(par[i])].append((i, int(wt[i])))
    dist = np.zeros((n, n), np.int64)
    for s in range(n):
        seen, stack = {s}, [(s, 0)]
        while stack:
            a, d = stack.pop()
            dist[order[s], order[a]] = d
            for b, k in adj[a]:
                if b not in seen:
                    seen.add(b)
                    stack.append((b, d + k))
    return dist
