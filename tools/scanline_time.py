"""Device time of the scan-line optimiser (smx_dev_scanline_wta_pair) beside semi-global matching (smx_dev_sgm_wta_pair) at a
pipeline shape (dev tool, GPU box):
python tools/scanline_time.py [workload] [repeats] [what ...]
what (default: sgm4 so4 sgm8 so8 step):
  sgm4, sgm8    the whole smx_dev_sgm_wta_pair call on the synthetic pair's census volumes, both views, paths 4 / 8, penalties
                127 / 382, with the S volumes and the states off: ms per call (host clock around 100 back-to-back calls ended by
                a synchronise), a figure per repeat
  so4, so8      smx_dev_scanline_wta_pair on the same volumes with the same penalties, tau_so 15, the gray pair as the guide
  step          PairPipeline.run with cost="census": aggregation "sgm", "scanline", "cross" and "cross-scanline" (their default
                parameters), alternating in this process
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/scanline_time.py kitti 1 so8`, one
`what` and nothing else per run (k_sgm_pack and k_sgm_select carry one name in both calls): the last 100 launches of each kernel
are the 100 timed calls (k_so_cols / k_sgm_cols: the last 200 / 600, two / six launches a call), and
`python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_s 100` reduces them."""
import ctypes as C
import sys
import time

import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import _lib, synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["sgm4", "so4", "sgm8", "so8", "step"]
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
so = PairPipeline(w, h, D, cost="census", aggregation="scanline")
so.run(dl, dr)                      # (its so_cost holds the census volumes of both views from here on)
torch.cuda.synchronize()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())
N = 100
for name in (k for k in which if k in ("sgm4", "sgm8", "so4", "so8")):
    paths = int(name[-1])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if name.startswith("sgm"):
        p = _lib.SgmParams()
        p.p1, p.p2, p.paths = 127, 382, paths
        ws_bytes = int(L.smx_sgm_workspace_bytes(w, h, D, 2))
        call = lambda: smx.check(L.smx_dev_sgm_wta_pair(C.byref(p), dp(so.so_cost[0]), dp(so.so_cost[1]), w, h, D, dp(so.keys),
                                                        None, None, dp(so.so_ws), ws_bytes, st))
    else:
        p = _lib.default_scanline_params()
        p.paths = paths
        call = lambda: smx.check(L.smx_dev_scanline_wta_pair(C.byref(p), dp(dl), dp(dr), 1, dp(so.so_cost[0]), dp(so.so_cost[1]),
                                                             w, h, D, so.dminl, so.dminr, dp(so.keys), None, None, None,
                                                             dp(so.so_ws), so.so_ws_bytes, st))
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    entry = "smx_dev_sgm_wta_pair" if name.startswith("sgm") else "smx_dev_scanline_wta_pair"
    print(f"{wl} {w}x{h}x{D} {entry} paths {paths} p1 {p.p1} p2 {p.p2} ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)


def step_ms(pipe, n=20):
    for _ in range(3):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


if "step" in which:
    pipes = {"scanline": so}
    for agg in ("sgm", "cross", "cross-scanline"):
        pipes[agg] = PairPipeline(w, h, D, cost="census", aggregation=agg)
    for _ in range(reps):
        print(f"{wl} census PairPipeline.run ms: " + "  ".join(f"{agg} {step_ms(pipes[agg]):.3f}"
                                                                 for agg in ("sgm", "scanline", "cross", "cross-scanline")), flush=True)
