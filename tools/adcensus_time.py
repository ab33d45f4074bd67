"""Device time of the AD-Census cost kernel at a pipeline shape (dev tool, GPU box):
python tools/adcensus_time.py [workload] [kernels|steps] [repeats]
  kernels  k_census_cost_pair, k_adcensus_cost_pair on the gray images and on colour images, both views per launch, the
           three alternating, `repeats` launches each after a warm-up.  Run it under
           `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adcensus_time.py kitti kernels` and
           read the trace with the `split` mode below.
  steps    PairPipeline(cost="adcensus").run against PairPipeline(cost="census").run, alternating inside every repeat; a
           host clock around N calls ended by a synchronise.
Both print the host-clock medians; the kernel times of record are the trace's:
python tools/adcensus_time.py split KERNEL_TRACE.csv
(needs no GPU) takes the trace of a `kernels` run apart by launch order -- per kernel 10 warm-up launches first, then the
timed ones, those of k_adcensus_cost_pair alternating gray, colour -- and prints median, minimum and maximum of each."""
import csv
import ctypes as C
import statistics
import sys
import time

if len(sys.argv) > 2 and sys.argv[1] == "split":
    runs = {"k_census_cost_pair": [], "k_adcensus_cost_pair": []}
    with open(sys.argv[2], newline="") as f:
        for r in csv.DictReader(f):
            for k in runs:
                if k in r["Kernel_Name"]:
                    runs[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    adc = sorted(runs["k_adcensus_cost_pair"])[20:]
    for name, ts in (("k_census_cost_pair", sorted(runs["k_census_cost_pair"])[10:]), ("k_adcensus_cost_pair gray", adc[0::2]),
                     ("k_adcensus_cost_pair colour", adc[1::2])):
        us = [(e - s) / 1e3 for s, e in ts]
        print(f"{name}: launches {len(us)} median {statistics.median(us):.2f} us min {min(us):.2f} max {max(us):.2f}")
    sys.exit(0)

import numpy as np
import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
mode = sys.argv[2] if len(sys.argv) > 2 else "kernels"
reps = int(sys.argv[3]) if len(sys.argv) > 3 else (30 if mode == "kernels" else 5)
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
imgs = torch.from_numpy(np.stack([Il, Ir])).cuda()
rgb = torch.from_numpy(np.stack([np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8) for g in (Il, Ir)])).cuda()
L = smx.lib()
dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
dminl, dminr = -(D - 1), 0


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def show(what, ms, extra=""):
    print(f"{wl} {w}x{h} D={D} {what}: median {statistics.median(ms):.4f} ms  (" + " ".join(f"{v:.4f}" for v in ms) + ")" + extra,
          flush=True)


if mode == "kernels":
    CP = smx.default_census_params()
    AP = [smx.default_adcensus_params(), smx.default_adcensus_params()]
    AP[1].colour = 1
    codes = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    cost = torch.empty((2, D, h, w), dtype=torch.float32, device="cuda")
    tabs = [torch.empty(64 + 766, dtype=torch.float32, device="cuda") for _ in AP]
    for p, t in zip(AP, tabs):
        smx.check(L.smx_dev_adcensus_tables(C.byref(p), dp(t), stream()))
    smx.check(L.smx_dev_census(C.byref(CP), dp(imgs), dp(codes), w, h, 2, stream()))
    gbytes = cost.numel() * 4 / 1e9

    def census_cost():
        smx.check(L.smx_dev_census_cost_pair(C.byref(CP), dp(codes), dp(cost[0]), dp(cost[1]), w, h, dminl, dminr, 0, D, stream()))

    def adc(k, il, ir, ch):
        smx.check(L.smx_dev_adcensus_cost_pair(C.byref(AP[k]), dp(tabs[k]), dp(codes), dp(il), dp(ir), ch, dp(cost[0]), dp(cost[1]),
                                               w, h, dminl, dminr, 0, D, stream()))

    cands = {"k_census_cost_pair": census_cost, "k_adcensus_cost_pair gray": lambda: adc(0, imgs[0], imgs[1], 1),
             "k_adcensus_cost_pair colour": lambda: adc(1, rgb[0], rgb[1], 3)}
    for fn in cands.values():
        for _ in range(10):
            fn()
    out = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            out[k].append(timed(fn, 1))
    for k, ms in out.items():
        print(f"{wl} {w}x{h} D={D} {k}: host clock around one launch and a synchronise, median {statistics.median(ms):.4f} ms "
              f"over {len(ms)} ({gbytes:.3f} GB of stores)", flush=True)
else:
    pa = PairPipeline(w, h, D, cost="adcensus")
    pc = PairPipeline(w, h, D, cost="census")
    cands = {"adcensus pair step": lambda: pa.run(imgs[0], imgs[1]), "census pair step": lambda: pc.run(imgs[0], imgs[1])}
    for fn in cands.values():
        for _ in range(5):
            fn()
    out = {k: [] for k in cands}
    for _ in range(reps):
        for k, fn in cands.items():
            out[k].append(timed(fn, 20))
    for k, ms in out.items():
        show(k, ms)
    pa.check_status()
    pc.check_status()
    print(f"ratio adcensus / census: {statistics.median(out['adcensus pair step']) / statistics.median(out['census pair step']):.3f}",
          flush=True)
