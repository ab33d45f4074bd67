"""Measurements of the ZNCC window cost at the KITTI shape (1242 x 375 x D 192), from the repository root:
python tools/zncc_time.py MODE [rx ry]   (profiles/zncc_kitti_kernel_times.txt).  Modes:
  kernels   smx_dev_zncc_moments, then smx_dev_census_cost_pair, smx_dev_mi_cost_pair and smx_dev_zncc_cost_pair over both
            whole volumes, alternating twice, 20 launches each after a warm-up call      (run under rocprofv3 --kernel-trace)
  cost      smx_dev_zncc_cost_pair alone, 20 launches                                    (run under rocprofv3 --pmc)
  pairs     smx_ctx_stereo_pair with the reference cost, the census cost and the ZNCC cost: host clock around the call
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


def main(mode, rx=3, ry=3):
    Il, Ir = synth.gen_pair(W, H, D, 7)
    zp = smx.default_zncc_params()
    zp.rx, zp.ry = rx, ry
    if mode in ("kernels", "cost"):
        imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
        cost = torch.empty((2, D, H, W), device="cuda")
        mom = torch.empty((2, H, W), dtype=torch.int64, device="cuda")
        zncc = lambda: _lib.check(L.smx_dev_zncc_cost_pair(C.byref(zp), dp(mom), dp(imgs[0]), dp(imgs[1]), dp(cost[0]), dp(cost[1]),
                                                           W, H, DMINL, DMINR, 0, D, st()))
        moments = lambda: _lib.check(L.smx_dev_zncc_moments(C.byref(zp), dp(imgs), dp(mom), W, H, 2, st()))
        timed(f"k_zncc_moments, both images, window {2 * rx + 1} x {2 * ry + 1}", moments)
        print(f"store floor: {2 * D * W * H * 4} bytes per cost call")
        if mode == "cost":
            timed(f"k_zncc_cost_pair, both views, 192 slices, window {2 * rx + 1} x {2 * ry + 1}", zncc)
            return
        codes = torch.empty((2, H, W), dtype=torch.int64, device="cuda")
        cp = _lib.default_census_params()
        _lib.check(L.smx_dev_census(C.byref(cp), dp(imgs), dp(codes), W, H, 2, st()))
        disp = torch.from_numpy(np.random.default_rng(1).integers(DMINL, 1, size=(H, W)).astype(np.float32)).cuda()
        hist = torch.empty((256, 256), dtype=torch.int32, device="cuda")
        _lib.check(L.smx_dev_mi_histogram(dp(imgs[0]), dp(imgs[1]), dp(disp), float(DMINL - 100), dp(hist), W, H, st()))
        table = torch.from_numpy(smx.mi_table(hist.cpu().numpy().view(np.uint32))).cuda()
        for rep in range(2):            # alternating, so that none always runs first
            timed("k_census_cost_pair, both views, 192 slices",
                  lambda: _lib.check(L.smx_dev_census_cost_pair(C.byref(cp), dp(codes), dp(cost[0]), dp(cost[1]), W, H, DMINL, DMINR, 0, D, st())))
            timed("k_mi_cost_pair, both views, 192 slices",
                  lambda: _lib.check(L.smx_dev_mi_cost_pair(dp(table), dp(imgs[0]), dp(imgs[1]), dp(cost[0]), dp(cost[1]), W, H, DMINL, DMINR, 0, D, st())))
            timed(f"k_zncc_cost_pair, both views, 192 slices, window {2 * rx + 1} x {2 * ry + 1}", zncc)
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
        _lib.check(L.smx_ctx_set_zncc(ctx, C.byref(zp)))
        clock(f"ZNCC pair, window {2 * rx + 1} x {2 * ry + 1}")
        _lib.check(L.smx_ctx_set_zncc(ctx, None))
    L.smx_destroy(ctx)


main(sys.argv[1], *(int(a) for a in sys.argv[2:4]))
