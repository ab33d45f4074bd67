// smx_tree_host.h -- the host arithmetic of the non-local tree filter (include/smx.h, above smx_tree_params): the parameter
// check, the two weight tables, the layout of the tree blob and the tree's build.  Plain C++ without HIP, so that
// tests/host_tree_check.cpp runs this very code under the sanitizers; the C entries (smx_capi.hip), the kernel (smx_tree.hip,
// which reads the layout) and the context (smx_ctx.hip) call it.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "smx.h"

#if defined(__HIPCC__)
#define SMX_TREE_HD __host__ __device__
#else
#define SMX_TREE_HD
#endif

namespace smx {

inline bool tree_params_ok(const smx_tree_params* p) { return p && isfinite(p->sigma) && p->sigma > 0.0; }

// t[k] = (float)exp(-k / sigma), u[k] = (float)(1 - exp(-2 k / sigma)), both in double; t[0] == 1 and u[0] == 0 whatever sigma is
inline void tree_tables(const smx_tree_params* p, float* t, float* u) {
    for (int k = 0; k < 256; ++k) {
        t[k] = (float)exp(-(double)k / p->sigma);
        u[k] = (float)(1.0 - exp(-2.0 * (double)k / p->sigma));
    }
}

// The byte offsets of the blob's arrays for a tree of n nodes (include/smx.h has the layout in words): the 4-byte arrays first,
// so that every one of them is 4-byte aligned in a 4-byte aligned blob, the two byte arrays behind them.
struct TreeLayout { size_t order, parent, child_first, level_start, child_count, wt, bytes; };
SMX_TREE_HD inline TreeLayout tree_layout(size_t n) {
    TreeLayout l;
    l.order = 8;
    l.parent = l.order + 4 * n;
    l.child_first = l.parent + 4 * n;
    l.level_start = l.child_first + 4 * n;
    l.child_count = l.level_start + 4 * (n + 1);
    l.wt = l.child_count + n;
    l.bytes = (l.wt + n + 3) & ~(size_t)3;
    return l;
}

// diff of two pixels of the guide: |dI| for one channel, the maximum over R, G, B for 3 or 4 (alpha is ignored)
inline int tree_diff(const uint8_t* a, const uint8_t* b, int ch) {
    int d = 0;
    for (int c = 0; c < (ch == 1 ? 1 : 3); ++c) {
        const int e = (int)a[c] - (int)b[c];
        const int m = e < 0 ? -e : e;
        d = m > d ? m : d;
    }
    return d;
}

// The tree of `guide` into `blob` (tree_layout(w * h).bytes bytes, every one of them written).  Kruskal over the edges in
// ascending (weight, id) order from a counting sort, then the breadth-first numbering from pixel 0.  It may throw
// std::bad_alloc: its three work arrays take 13 bytes a pixel.
inline void tree_build(const uint8_t* guide, int ch, int w, int h, uint8_t* blob) {
    const size_t n = (size_t)w * h;
    const TreeLayout lay = tree_layout(n);
    memset(blob, 0, lay.bytes);
    uint32_t* const head = (uint32_t*)blob;
    uint32_t* const order = (uint32_t*)(blob + lay.order);
    uint32_t* const parent = (uint32_t*)(blob + lay.parent);
    uint32_t* const child_first = (uint32_t*)(blob + lay.child_first);
    uint32_t* const level_start = (uint32_t*)(blob + lay.level_start);
    uint8_t* const child_count = blob + lay.child_count;
    uint8_t* const wt = blob + lay.wt;
    auto px = [&](size_t p) { return guide + p * (size_t)ch; };

    // the edges by (weight, id): edge 2p joins p and p + 1, edge 2p + 1 joins p and p + w
    size_t at[257] = {};
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = (size_t)y * w + x;
            if (x < w - 1) ++at[tree_diff(px(p), px(p + 1), ch) + 1];
            if (y < h - 1) ++at[tree_diff(px(p), px(p + w), ch) + 1];
        }
    for (int k = 0; k < 256; ++k) at[k + 1] += at[k];
    std::vector<uint32_t> edges(at[256]);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = (size_t)y * w + x;
            if (x < w - 1) edges[at[tree_diff(px(p), px(p + 1), ch)]++] = (uint32_t)(2 * p);
            if (y < h - 1) edges[at[tree_diff(px(p), px(p + w), ch)]++] = (uint32_t)(2 * p + 1);
        }

    // Kruskal; link[p]: bit 0 the edge (p, p + 1) is in the tree, bit 1 the edge (p, p + w)
    std::vector<uint32_t> up(n);
    std::vector<uint8_t> link(n, 0);
    for (size_t p = 0; p < n; ++p) up[p] = (uint32_t)p;
    auto find = [&](uint32_t a) {
        while (up[a] != a) { up[a] = up[up[a]]; a = up[a]; }
        return a;
    };
    size_t taken = 0;
    for (size_t k = 0; k < edges.size() && taken + 1 < n; ++k) {
        const uint32_t e = edges[k], p = e >> 1, q = p + ((e & 1) ? (uint32_t)w : 1u);
        const uint32_t a = find(p), b = find(q);
        if (a == b) continue;
        up[a < b ? b : a] = a < b ? a : b;
        link[p] |= (e & 1) ? 2 : 1;
        ++taken;
    }

    // breadth first from pixel 0; the children of a node in ascending pixel index: up, left, right, down
    order[0] = 0;
    parent[0] = 0;
    size_t tail = 1, i = 0;
    uint32_t level = 0;
    level_start[0] = 0;
    level_start[1] = 1;
    for (;;) {
        for (; i < level_start[level + 1]; ++i) {
            const uint32_t p = order[i], par = i ? order[parent[i]] : 0xFFFFFFFFu;
            const int y = (int)(p / (uint32_t)w), x = (int)(p - (uint32_t)y * (uint32_t)w);
            const size_t first = tail;
            auto child = [&](uint32_t q) {
                if (q == par) return;
                order[tail] = q;
                parent[tail] = (uint32_t)i;
                wt[tail] = (uint8_t)tree_diff(px(p), px(q), ch);
                ++tail;
            };
            if (y > 0 && (link[p - (uint32_t)w] & 2)) child(p - (uint32_t)w);
            if (x > 0 && (link[p - 1] & 1)) child(p - 1);
            if (x < w - 1 && (link[p] & 1)) child(p + 1);
            if (y < h - 1 && (link[p] & 2)) child(p + (uint32_t)w);
            child_first[i] = (uint32_t)first;
            child_count[i] = (uint8_t)(tail - first);
        }
        if (tail == level_start[level + 1]) break;
        ++level;
        level_start[level + 1] = (uint32_t)tail;
    }
    head[0] = (uint32_t)n;
    head[1] = level + 1;
}

}  // namespace smx
