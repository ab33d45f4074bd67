"""Measurements of the MI cost at the KITTI shape (1242 x 375 x D 192), from the repository root: python tools/mi_time.py MODE
(profiles/mi_kitti_kernel_times.txt).  Modes:
  kernels   histogram (natural map), smx_dev_census_cost_pair and smx_dev_mi_cost_pair, 20 launches each  (run under rocprofv3)
  flat      histogram of a flat pair with one constant label, 20 launches                                 (run under rocprofv3)
  pairs     smx_ctx_stereo_pair with the census cost and with MI at 1, 2, 3 tables: host clock around the synchronous call
"""
import ctypes as C
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

W, H, D = 1242, 375, 192
DMINL, DMINR = -(D - 1), 0
L = smx.lib()


def dp(t):
    return C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def timed(name, fn, reps=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    print(f"{name}: {a.elapsed_time(b) / reps * 1000:.1f} us per call over {reps} calls (device events)", flush=True)


def main(mode):
    Il, Ir = synth.gen_pair(W, H, D, 7)
    if mode in ("kernels", "flat"):
        if mode == "flat":
            Il, Ir = np.full((H, W), 131, np.uint8), np.full((H, W), 77, np.uint8)
            disp = np.full((H, W), -3, np.float32)
        else:
            disp = np.random.default_rng(1).integers(DMINL, 1, size=(H, W)).astype(np.float32)
            disp[np.random.default_rng(2).random((H, W)) < 0.2] = DMINL - 100
        il, ir, m = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda(), torch.from_numpy(disp).cuda()
        hist = torch.empty((256, 256), dtype=torch.int32, device="cuda")
        timed(f"histogram ({mode}) memset + k_mi_histogram",
              lambda: _lib.check(L.smx_dev_mi_histogram(dp(il), dp(ir), dp(m), float(DMINL - 100), dp(hist), W, H, st())))
        print("counted", int(hist.sum().item()), "max counter", int(hist.max().item()))
        if mode == "flat":
            return
        table = torch.from_numpy(smx.mi_table(hist.cpu().numpy().view(np.uint32))).cuda()
        cost = torch.empty((2, D, H, W), device="cuda")
        imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
        codes = torch.empty((2, H, W), dtype=torch.int64, device="cuda")
        cp = _lib.default_census_params()
        _lib.check(L.smx_dev_census(C.byref(cp), dp(imgs), dp(codes), W, H, 2, st()))
        nbytes = 2 * D * W * H * 4
        print(f"store floor: {nbytes} bytes per call")
        for rep in range(2):            # alternating, so that neither always runs first
            timed("k_census_cost_pair, both views, 192 slices",
                  lambda: _lib.check(L.smx_dev_census_cost_pair(C.byref(cp), dp(codes), dp(cost[0]), dp(cost[1]), W, H, DMINL, DMINR, 0, D, st())))
            timed("k_mi_cost_pair, both views, 192 slices",
                  lambda: _lib.check(L.smx_dev_mi_cost_pair(dp(table), dp(imgs[0]), dp(imgs[1]), dp(cost[0]), dp(cost[1]), W, H, DMINL, DMINR, 0, D, st())))
        return
    # pairs
    ctx = C.c_void_p()
    _lib.check(L.smx_create(C.byref(smx.default_params()), W, H, D, C.byref(ctx)))
    bufs = {k: np.empty((H, W), np.float32) for k in ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")}
    out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})

    def pair():
        _lib.check(L.smx_ctx_stereo_pair(ctx, Il.ctypes.data, Ir.ctypes.data, DMINL, DMINR, C.byref(out)))

    def clock(name, reps=5):
        pair()
        pair()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pair()
            ts.append((time.perf_counter() - t0) * 1e3)
        print(f"{name}: median {sorted(ts)[len(ts) // 2]:.2f} ms, min {min(ts):.2f}, max {max(ts):.2f} over {reps} pairs (host clock, "
              "uploads and downloads included)", flush=True)

    for rnd in range(2):
        clock("plain pair (reference cost)")
        _lib.check(L.smx_ctx_set_cost(ctx, 1, None))
        clock("census pair")
        for it in (1, 2, 3):
            p = smx.default_mi_params()
            p.iterations = it
            _lib.check(L.smx_ctx_set_mi(ctx, C.byref(p)))
            clock(f"MI pair, {it} table(s), random start")
        p = smx.default_mi_params()
        p.init = 1
        _lib.check(L.smx_ctx_set_mi(ctx, C.byref(p)))
        clock("MI pair, 3 tables, reference start")
        _lib.check(L.smx_ctx_set_cost(ctx, 0, None))
    L.smx_destroy(ctx)


main(sys.argv[1])
