"""Device time of the cross-based aggregation (smx_dev_cross_wta_pair) at a pipeline shape (dev tool, GPU box):
python tools/cross_time.py [workload] [repeats] [what ...]
what (default: call step):
  call          the whole smx_dev_cross_wta_pair call on the AD-Census volumes of the synthetic pair, both views, with the
                aggregated volumes and the states off, every slice the workspace bound admits in flight, Mei's parameters: 10
                warm-up calls, then ms per call (host clock around 30 back-to-back calls ended by a synchronise), a figure
                per repeat
  step          PairPipeline.run with cost="adcensus": aggregation="cross" at 4 iterations and at 1 iteration against
                guidance="rgb" and aggregation="sgm", alternating inside each repeat
  trace CSV     no GPU: reduces the kernel trace of a `call` run.  A call is a fixed sequence of launches (the arms, the four
                area passes, then per chunk two passes per iteration and the winner-take-all pass), so the launches are reduced
                by their position in the call: median, minimum and maximum over the last 30 calls, in microseconds
The colour guide of the synthetic pair is its gray image in three channels, (g, g // 2 + 60, 255 - g).
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cross_time.py kitti 1 call`, one
`what` and nothing else per run; then `python tools/cross_time.py kitti 1 trace DIR/*/*kernel_trace.csv`."""
import ctypes as C
import sys
import time

import numpy as np

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["call", "step"]
WARM, N = 10, 30

if which[0] == "trace":
    import csv
    import statistics
    rows = []
    with open(which[1], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_cross_" in name or "k_wta" in name:
                short = name.replace("(anonymous namespace)::", "").replace("smx::", "").removeprefix("void ").split("(")[0]
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "k_cross_arms" in r[2]]
    per = starts[1] - starts[0]
    assert all(b - a == per for a, b in zip(starts, starts[1:])) and len(rows) == per * len(starts), "not a trace of `call` alone"
    calls = [rows[i:i + per] for i in starts][-N:]
    total = 0.0
    print(f"{len(starts)} calls of {per} launches, the last {len(calls)} taken")
    for k in range(per):
        us = [(c[k][1] - c[k][0]) / 1e3 for c in calls]
        total += statistics.median(us)
        print(f"  {k:2d} {calls[0][k][2]:<40} median {statistics.median(us):9.2f} min {min(us):9.2f} max {max(us):9.2f}")
    print(f"sum of medians {total:.2f}")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
colour = lambda g: np.ascontiguousarray(np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
cl, cr = torch.from_numpy(colour(Il)).cuda(), torch.from_numpy(colour(Ir)).cuda()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())


def cross_params(iterations):
    p = smx.default_cross_params()
    p.iterations = iterations
    return p


big = dict(cost="adcensus", max_ws_bytes=16 << 30)
pipes = {"cross4": PairPipeline(w, h, D, aggregation="cross", cross_params=cross_params(4), **big)}
if "step" in which:
    pipes["cross1"] = PairPipeline(w, h, D, aggregation="cross", cross_params=cross_params(1), **big)
    pipes["rgb"] = PairPipeline(w, h, D, guidance="rgb", **big)
    pipes["sgm"] = PairPipeline(w, h, D, aggregation="sgm", **big)


def run(name):
    if name == "sgm":
        pipes[name].run(dl, dr)
    else:
        pipes[name].run(dl, dr, rgb_l=cl, rgb_r=cr)


for name in pipes:
    run(name)
torch.cuda.synchronize()
x = pipes["cross4"]
print(f"{wl} {w}x{h}x{D} aggregation=cross: {x.slices_in_flight} slices in flight, workspace {x.cross_ws_bytes / 2**20:.0f} MiB",
      flush=True)

if "call" in which:
    # the AD-Census volumes of the pair, whole
    P = smx.default_adcensus_params()
    vol = torch.empty((2, D, h, w), dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    smx.check(L.smx_dev_adcensus_cost_pair(C.byref(P), dp(x.adcensus_table), dp(x.codes), dp(dl), dp(dr), 1, dp(vol[0]), dp(vol[1]),
                                           w, h, x.dminl, x.dminr, 0, D, st))
    X = cross_params(4)
    call = lambda: smx.check(L.smx_dev_cross_wta_pair(C.byref(X), dp(cl), dp(cr), 3, dp(vol[0]), dp(vol[1]), w, h, 0, D,
                                                      dp(x.keys), None, None, None, dp(x.cross_ws), x.cross_ws_bytes, st))
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    print(f"{wl} {w}x{h}x{D} smx_dev_cross_wta_pair l1 {X.l1} l2 {X.l2} tau {X.tau1}/{X.tau2} iterations {X.iterations} ms/call "
          + " ".join(f"{v:.4f}" for v in ms), flush=True)


def step_ms(name):
    for _ in range(3):
        run(name)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        run(name)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3


if "step" in which:
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} PairPipeline.run cost=adcensus ms: " + "  ".join(f"{name} {step_ms(name):.4f}" for name in pipes), flush=True)
