"""Device time of the census / Hamming cost kernels at a pipeline shape (dev tool, GPU box):
python tools/census_time.py [workload] [repeats]
Prints, alternating the candidates inside every repeat (same box, same session):
  1. k_census_cost_pair (both views, one launch) against the two smx_dev_cost_volume launches of the reference cost
     for the same shape, ms per call and GB/s of stores;
  2. k_census for the pair, ms per call;
  3. a whole census pair step (PairPipeline(cost="census").run) against the materialised-cost flow of the reference cost
     (cost volumes built before the timed region, aggregate from them + finish: bench.py --full --source cost).
Times: a host clock around N calls ended by a synchronise.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`
(kernels k_census, k_census_cost_pair, k_cost)."""
import ctypes as C
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
L = smx.lib()
dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
P, CP = smx.default_params(), smx.default_census_params()
dminl, dminr = -(D - 1), 0
codes = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
cost = torch.empty((2, D, h, w), dtype=torch.float32, device="cuda")
gbytes = cost.numel() * 4 / 1e9


def census():
    smx.check(L.smx_dev_census(C.byref(CP), dp(imgs), dp(codes), w, h, 2, stream()))


def census_cost():
    smx.check(L.smx_dev_census_cost_pair(C.byref(CP), dp(codes), dp(cost[0]), dp(cost[1]), w, h, dminl, dminr, 0, D, stream()))


def reference_cost():
    smx.check(L.smx_dev_cost_volume(C.byref(P), dp(imgs[0]), dp(imgs[1]), dp(cost[0]), w, w, h, dminl, 0, D, stream()))
    smx.check(L.smx_dev_cost_volume(C.byref(P), dp(imgs[1]), dp(imgs[0]), dp(cost[1]), w, w, h, dminr, 0, D, stream()))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def compare(cands, n, warm):
    """{name: [ms per repeat]}, the candidates alternating inside every repeat."""
    for fn in cands.values():
        for _ in range(warm):
            fn()
    out = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            out[k].append(timed(fn, n))
    return out


def show(what, ms, extra=""):
    print(f"{wl} {w}x{h} D={D} {what}: median {statistics.median(ms):.4f} ms  (" + " ".join(f"{v:.4f}" for v in ms) + ")" + extra,
          flush=True)


census()
r = compare({"census_cost_pair": census_cost, "reference_cost_x2": reference_cost}, 50, 10)
for k, ms in r.items():
    show(k, ms, f"  {gbytes / statistics.median(ms) * 1e3:.0f} GB/s of stores")
print(f"ratio census / reference: {statistics.median(r['census_cost_pair']) / statistics.median(r['reference_cost_x2']):.3f}", flush=True)
show("k_census (pair)", compare({"c": census}, 200, 20)["c"])

pc = PairPipeline(w, h, D, cost="census")
pr = PairPipeline(w, h, D)
cl, cr = pr.cost_volumes(imgs[0], imgs[1])


def census_step():
    pc.run(imgs[0], imgs[1])


def reference_step():
    pr.aggregate(imgs[0], imgs[1], cl, cr)
    pr.finish()


r = compare({"census pair step": census_step, "reference step from materialised costs": reference_step}, 20, 5)
for k, ms in r.items():
    show(k, ms)
pc.check_status()
pr.check_status()
print(f"difference: {statistics.median(r['census pair step']) - statistics.median(r['reference step from materialised costs']):.4f} ms "
      f"(the census step also builds its codes and its cost volumes)", flush=True)
