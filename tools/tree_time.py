"""Time of the non-local tree filter (smx_tree_build, smx_dev_tree_wta_pair, smx_ctx_set_tree) at a pipeline shape, with the
permeability filter as the yardstick of the same job (dev tool, GPU box):  python tools/tree_time.py [workload] [repeats] [what]
what (default: filter):
  build     smx_tree_build on the synthetic pair's two gray images, host only: ms per view by the host clock, a figure per
            repeat, and the levels of the two trees
  filter    smx_dev_tree_wta_pair and smx_dev_permeability_wta_pair alternately inside each repeat, both views of the workload's
            shape, random volumes, default sigmas, the guides the synthetic pair's gray images, each with a workspace for every
            slice at once up to 1 GiB (what the context takes): 2 warm-up calls, then 10 back-to-back calls ended by a
            synchronise, ms per call by the host clock.  The filtered volumes go to a buffer of their own, so that every call
            filters the same values
  pair      a whole smx_ctx_stereo_pair with the tree filter on and with the permeability filter on, two contexts, alternately
            inside each repeat, 5 calls each after one warm-up: ms per pair by the host clock (the host build of the two trees
            included)
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/tree_time.py kitti 1 filter`, one
`what` and nothing else per run; then `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_tree_filter 10` (k_wta,
k_perm_h, k_perm_v, k_perm_weights)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import _lib, synth  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
what = sys.argv[3] if len(sys.argv) > 3 else "filter"

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
L = smx.lib()
dminl = -(D - 1)

if what == "build":
    nbytes = L.smx_tree_bytes(w, h)
    blobs = [np.zeros(nbytes // 4, np.uint32) for _ in range(2)]
    for _ in range(reps):
        ms = []
        for g, b in zip((Il, Ir), blobs):
            t0 = time.perf_counter()
            smx.check(L.smx_tree_build(g.ctypes.data, 1, w, h, b.ctypes.data))
            ms.append((time.perf_counter() - t0) * 1e3)
        print(f"{wl} {w}x{h} smx_tree_build ms per view: " + " ".join(f"{x:.2f}" for x in ms) +
              f"; levels {int(blobs[0][1])} {int(blobs[1][1])}, {w * h} nodes, blob {nbytes} bytes", flush=True)
    sys.exit(0)

import torch  # noqa: E402

vp = lambda t: C.c_void_p(t.data_ptr())


def timed(call, warm, n):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


if what == "filter":
    dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
    trees = torch.stack([torch.from_numpy(smx.tree_build(g)) for g in (Il, Ir)]).cuda()
    levels = [int(smx.tree_build(g)[4:8].view(np.uint32)[0]) for g in (Il, Ir)]
    g = torch.Generator(device="cuda").manual_seed(1)
    vol = torch.randn((2, D, h, w), device="cuda", generator=g)
    out = torch.empty_like(vol)
    keys = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    per = 2 * w * h * 4
    tchunk = min(D, max(1, (1 << 30) // per))
    pchunk = min(D, max(1, (1 << 30) // per - 2))
    tws = torch.empty(per * tchunk, dtype=torch.uint8, device="cuda")
    pws = torch.empty(per * (2 + pchunk), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tp, pp = smx.default_tree_params(), smx.default_perm_params()

    def tree():
        smx.check(L.smx_dev_tree_wta_pair(C.byref(tp), vp(vol[0]), vp(vol[1]), vp(trees[0]), vp(trees[1]), w, h, dminl, 0, D, vp(keys),
                                          vp(out), None, None, vp(tws), tws.numel(), st))

    def perm():
        smx.check(L.smx_dev_permeability_wta_pair(C.byref(pp), vp(vol[0]), vp(vol[1]), vp(dl), vp(dr), 1, w, h, dminl, 0, D, vp(keys),
                                                  vp(out), None, None, vp(pws), pws.numel(), st))

    print(f"{wl} {w}x{h}x{D}: trees of {levels} levels ({w * h // levels[0]} nodes a level), {tchunk} slices a chunk, "
          f"{2 * D} workgroups a call", flush=True)
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} ms/call: smx_dev_tree_wta_pair {timed(tree, 2, 10):.4f}  smx_dev_permeability_wta_pair {timed(perm, 2, 10):.4f}",
              flush=True)
else:
    bufs = {k: np.empty((h, w), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
    ctxs = {}
    for name in ("tree", "permeability"):
        ctx = C.c_void_p()
        smx.check(L.smx_create(C.byref(smx.default_params()), w, h, D, C.byref(ctx)))
        if name == "tree":
            smx.check(L.smx_ctx_set_tree(ctx, C.byref(smx.default_tree_params())))
        else:
            smx.check(L.smx_ctx_set_permeability(ctx, C.byref(smx.default_perm_params())))
        ctxs[name] = ctx
    maps = {}
    for _ in range(reps):       # alternating, in one session
        line = []
        for name, ctx in ctxs.items():
            call = lambda: smx.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, dminl, 0, C.byref(out)))
            line.append(f"{name} {timed(call, 1, 5):.3f}")
            maps[name] = bufs["dmap_l"].copy()
        print(f"{wl} {w}x{h}x{D} smx_ctx_stereo_pair ms: " + "  ".join(line), flush=True)
    print(f"{wl} left winners that differ between the two modes: {int((maps['tree'] != maps['permeability']).sum())} of {w * h}",
          flush=True)
    for ctx in ctxs.values():
        L.smx_destroy(ctx)
