// smx_tree.hip -- the non-local tree filter (Yang, CVPR 2012; not a stage of the reference: opt-in).  The definition is the
// comment above smx_tree_params in include/smx.h and tests/tree_ref.py, bit for bit: every product and sum of the two sweeps
// rounded to f32 on its own, in the order of the definition, whatever the launch geometry.
//
//   k_tree_filter   one workgroup per (slice of the chunk, view).  The tree comes as the host-built blob in breadth-first order
//                   (smx_tree_host.h), the two tables t and u as kernel arguments staged in LDS.  The workgroup walks the levels
//                   with one __syncthreads() a level -- every thread the same trip count -- a thread a node of the level, in a
//                   stride loop where a level is wider than the workgroup.  U and A live in ONE breadth-first-ordered plane of
//                   the workspace per slice in flight: up, levels descending, U[i] = C[order[i]] + sum over its children, which
//                   lie side by side in the level below; down, levels ascending, A[i] = t A[parent] + u U[i] written over U[i],
//                   whose last reader is this very thread, and scattered to out[order[i]].  Only the gather of C and the scatter
//                   of out go through order; every other access is contiguous along the level.
//
// out may be the input volume: the last read of C (the up sweep) lies a barrier before the first write of out (the down sweep),
// and a workgroup touches its own slice only.  No atomics, no grid-wide synchronisation, no flags between workgroups, no
// transcendental, no floating-point division.  The blob is read-only device memory that the kernel does not trust blindly: an
// index past the tree is skipped, so that a wrong blob gives wrong numbers and never an access outside the buffers of the call.
// The winners come from wta_launch (smx_wta.h) over the filtered slices of each chunk.
//
// Must be compiled with -ffp-contract=off.
#include "smx_api.h"
#include "smx_launch.h"
#include "smx_wta.h"

namespace smx {
namespace {

constexpr int TREE_NT = 256;    // threads of a workgroup: a node of the level each

struct TreeTables { float t[256], u[256]; };

struct TreeArgs {
    const float* in[2];         // per view: the first slice of the chunk
    float* out[2];              // may be in[]
    float* bfs[2];              // the chunk's breadth-first planes
    const uint8_t* tree[2];     // the views' blobs
    uint32_t n;                 // w * h: the nodes of a tree
};

// grid (slices of the chunk, views)
__global__ __launch_bounds__(TREE_NT) void k_tree_filter(TreeArgs a, TreeTables tab) {
    __shared__ float t[256], u[256];
    {   // (a kernel argument is not indexed by the lane: every lane picks its entries out of the uniform values)
        float mt = 0.0f, mu = 0.0f;
#pragma unroll
        for (int k = 0; k < 256; ++k) {
            mt = (int)threadIdx.x == k ? tab.t[k] : mt;
            mu = (int)threadIdx.x == k ? tab.u[k] : mu;
        }
        t[threadIdx.x] = mt;
        u[threadIdx.x] = mu;
    }
    __syncthreads();
    const int v = (int)blockIdx.y;
    const uint32_t n = a.n, tid = threadIdx.x;
    const uint8_t* blob = a.tree[v];
    const TreeLayout lay = tree_layout(n);
    const uint32_t* order = (const uint32_t*)(blob + lay.order);
    const uint32_t* parent = (const uint32_t*)(blob + lay.parent);
    const uint32_t* child_first = (const uint32_t*)(blob + lay.child_first);
    const uint32_t* level_start = (const uint32_t*)(blob + lay.level_start);
    const uint8_t* child_count = blob + lay.child_count;
    const uint8_t* wt = blob + lay.wt;
    const size_t base = (size_t)blockIdx.x * n;
    const float* in = a.in[v] + base;       // (not restrict: out may be in)
    float* out = a.out[v] + base;
    float* bfs = a.bfs[v] + base;
    uint32_t levels = __builtin_amdgcn_readfirstlane(((const uint32_t*)blob)[1]);
    levels = levels < n ? levels : n;
    auto bound = [&](uint32_t l) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(level_start[l]);
        return s < n ? s : n;
    };
    // up: a node takes its own cost, then its children's sums in ascending order
    for (uint32_t l = levels; l-- > 0;) {
        const uint32_t b = bound(l), e = bound(l + 1);
        for (uint32_t i = b + tid; i < e; i += TREE_NT) {
            const uint32_t o = order[i], cf = child_first[i], cc = child_count[i];
            float s = o < n ? in[o] : 0.0f;
            for (uint32_t c = cf; c < cf + cc && c < n; ++c) {
                const float p = t[wt[c]] * bfs[c];
                s = s + p;
            }
            bfs[i] = s;
        }
        __syncthreads();
    }
    // down: a node mixes its parent's result with its own sum
    for (uint32_t l = 0; l < levels; ++l) {
        const uint32_t b = bound(l), e = bound(l + 1);
        for (uint32_t i = b + tid; i < e; i += TREE_NT) {
            const uint32_t o = order[i];
            float r = bfs[i];
            if (i != 0) {
                const uint32_t pa = parent[i], k = wt[i];
                const float fromp = t[k] * bfs[pa < i ? pa : 0];
                const float own = u[k] * r;
                r = fromp + own;
                bfs[i] = r;
            }
            if (o < n) out[o] = r;
        }
        __syncthreads();
    }
}

// the floats of one view's plane
inline size_t plane_bytes(int w, int h) { return (size_t)w * h * sizeof(float); }

}  // namespace

// Per view and slice in flight: the breadth-first plane, and a plane of the filtered slice for the calls that keep no volume.
// Sized for those: a call with d_out gets by with half.
size_t tree_workspace_bytes(int w, int h, int nslices, int nviews) {
    return (size_t)nviews * plane_bytes(w, h) * 2 * (size_t)nslices;
}

int tree_chunk(int w, int h, int nviews, size_t ws_bytes, int count, bool own_out, int max_chunk) {
    const size_t per = (size_t)nviews * plane_bytes(w, h);
    size_t k = ws_bytes / per / (own_out ? 2 : 1);
    if (k > (size_t)count) k = (size_t)count;
    if (k > 65535) k = 65535;           // (kept to the bound of the other chunked entries)
    if (max_chunk > 0 && k > (size_t)max_chunk) k = (size_t)max_chunk;
    return (int)k;
}

int launch_tree_wta_pair(const float* t, const float* u, const float* vol_l, const float* vol_r, const uint8_t* tree_l,
                         const uint8_t* tree_r, int w, int h, int size_d, int64_t* keys, float* out, float* nbr, float* uq, void* ws,
                         int chunk, hipStream_t st) {
    const size_t n = (size_t)w * h;
    const float* vols[2] = {vol_l, vol_r};
    const uint8_t* trees[2] = {tree_l, tree_r};
    const int both = vol_l && vol_r ? 1 : 0;
    // view k of the V given ones; with both views the outputs hold the left view first, a single view lies at the front
    int V = 0;
    const float* vin[2] = {};
    const uint8_t* vtree[2] = {};
    float* vout[2] = {};
    int64_t* vkeys[2] = {};
    float *vnbr[2] = {}, *vuq[2] = {};
    for (int view = 0; view < 2; ++view) {
        if (!vols[view]) continue;
        const size_t slot = both ? (size_t)view : 0;
        vin[V] = vols[view];
        vtree[V] = trees[view];
        vout[V] = out ? out + slot * size_d * n : nullptr;
        vkeys[V] = keys ? keys + slot * n : nullptr;
        vnbr[V] = nbr ? nbr + slot * 3 * n : nullptr;
        vuq[V] = uq ? uq + slot * 3 * n : nullptr;
        ++V;
    }
    float* const bfs = (float*)ws;                               // [V][chunk][n]
    float* const own = bfs + (size_t)V * chunk * n;              // [V][chunk][n], used where out is NULL
    TreeTables tab;
    for (int k = 0; k < 256; ++k) { tab.t[k] = t[k]; tab.u[k] = u[k]; }
    for (int s0 = 0; s0 < size_d; s0 += chunk) {
        const int cnt = s0 + chunk < size_d ? chunk : size_d - s0;
        TreeArgs ta = {};
        ta.n = (uint32_t)n;
        const float* q[2] = {};
        for (int k = 0; k < V; ++k) {
            float* dst = vout[k] ? vout[k] + (size_t)s0 * n : own + (size_t)k * chunk * n;
            ta.in[k] = vin[k] + (size_t)s0 * n;
            ta.out[k] = dst;
            ta.bfs[k] = bfs + (size_t)k * chunk * n;
            ta.tree[k] = vtree[k];
            q[k] = dst;
        }
        hipLaunchKernelGGL(k_tree_filter, dim3((unsigned)cnt, (unsigned)V), dim3(TREE_NT), 0, st, ta, tab);
        SMX_HIP(hipGetLastError());
        if (keys)
            if (int rc = wta_launch(WTA_NATURAL, V, q, vkeys, nbr ? vnbr : nullptr, uq ? vuq : nullptr, w, h, n, cnt, s0, nullptr, 0,
                                    s0 == 0, st))
                return rc;
    }
    return SMX_OK;
}

}  // namespace smx
