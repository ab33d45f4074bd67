"""Device time of hierarchical belief propagation (smx_dev_bp_wta_pair) at a pipeline shape (dev tool, GPU box):
python tools/bp_time.py [workload] [repeats] [what ...]
what (default: call step):
  call      the whole smx_dev_bp_wta_pair call on the synthetic pair's census volumes, both views, at the defaults, with the S
            volumes and the states off: 10 + 100 back-to-back calls; ms per call (host clock around the 100, ended by a
            synchronise), a figure per repeat.  The workspace, the levels' sizes and the bytes a level-0 iteration asks for
            are printed too
  sgm       the first yardstick: smx_dev_sgm_wta_pair at 8 paths on the same volumes, 10 + 100 calls
  wta       the second yardstick: PairPipeline(want_agg=True).run on the synthetic pair, 10 + 100 times -- its trace holds the
            natural-order winner-take-all pass over the materialised volumes of the same shape (k_wta<Natural, ..>)
  step      PairPipeline.run with cost="census": aggregation="bp" against aggregation="sgm", alternating in this process
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bp_time.py kitti 1 call`, one
`what` and nothing else per run, then
  python tools/bp_time.py trace DIR/*/*kernel_trace.csv [substring of the kernel names, default k_bp_] [calls taken, default 100]
reduces the trace: the number of calls is the smallest launch count among the kernels that hold the substring, and the launches
of every kernel whose count is a multiple of it are dealt, in start order, to the calls; a kernel launched several times a call
(k_bp_iter: iterations x levels, k_bp_coarse, k_bp_spread) gets a line per position in the call, since the levels differ in
size.  Per line the median over the last 100 calls, and at the end the sum of the medians: the device time of a call."""
import collections
import csv
import ctypes as C
import statistics
import sys
import time

CALLS = 110


def reduce_trace(path, pattern, taken):
    runs = collections.defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            runs[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    calls = min(len(ts) for name, ts in runs.items() if pattern in name)
    print(f"{calls} calls in the trace")
    total = 0.0
    for name, ts in sorted(runs.items(), key=lambda kv: min(kv[1])):
        if len(ts) % calls:
            continue                    # (not a kernel of the timed calls)
        ts.sort()
        per = len(ts) // calls
        short = name.replace("(anonymous namespace)::", "").removeprefix("void ").split("(")[0]
        for k in range(per):
            us = [(e - s) / 1e3 for s, e in ts[k::per][-taken:]]
            total += statistics.median(us)
            print(f"{short:<28} launch {k + 1:>2} of {per:<2} a call: median {statistics.median(us):9.2f} us  min {min(us):9.2f}  "
                  f"max {max(us):9.2f}  ({len(us)} calls)")
    print(f"sum of medians {total:.2f} us")


if len(sys.argv) > 2 and sys.argv[1] == "trace":
    reduce_trace(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "k_bp_", int(sys.argv[4]) if len(sys.argv) > 4 else 100)
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import _lib, synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["call", "step"]
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())


def timed(call, label):
    for _ in range(10):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(CALLS - 10):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / (CALLS - 10) * 1e3)
    print(f"{wl} {w}x{h}x{D} {label} ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)


def step_ms(pipe):
    for _ in range(3):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3


for what in which:
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if what == "call":
        pipe = PairPipeline(w, h, D, cost="census", aggregation="bp")
        pipe.run(dl, dr)
        p = pipe.bp_params
        dpad = (D + 63) // 64 * 64
        sizes, lw, lh = [], w, h
        for _ in range(p.levels):
            sizes.append((lw, lh))
            lw, lh = (lw + 1) // 2, (lh + 1) // 2
        print(f"{wl} workspace {pipe.bp_ws_bytes} bytes for both views; levels {sizes}; a level-0 iteration asks for "
              f"{2 * (w * h // 2) * dpad * (1 + 8 + 8)} bytes for both views", flush=True)
        timed(lambda: smx.check(L.smx_dev_bp_wta_pair(C.byref(p), dp(pipe.bp_cost[0]), dp(pipe.bp_cost[1]), w, h, D, dp(pipe.keys),
                                                      None, None, None, dp(pipe.bp_ws), pipe.bp_ws_bytes, st)),
              f"smx_dev_bp_wta_pair step {p.step} trunc {p.trunc} iterations {p.iterations} levels {p.levels}")
    elif what == "sgm":
        pipe = PairPipeline(w, h, D, cost="census", aggregation="sgm")
        pipe.run(dl, dr)
        p = pipe.sgm_params
        timed(lambda: smx.check(L.smx_dev_sgm_wta_pair(C.byref(p), dp(pipe.sgm_cost[0]), dp(pipe.sgm_cost[1]), w, h, D,
                                                       dp(pipe.keys), None, None, dp(pipe.sgm_ws), pipe.sgm_ws_bytes, st)),
              f"smx_dev_sgm_wta_pair paths {p.paths}")
    elif what == "wta":
        pipe = PairPipeline(w, h, D, want_agg=True)
        timed(lambda: pipe.run(dl, dr), "PairPipeline(want_agg=True).run")
    elif what == "step":
        bp = PairPipeline(w, h, D, cost="census", aggregation="bp")
        sgm = PairPipeline(w, h, D, cost="census", aggregation="sgm")
        for _ in range(reps):
            print(f"{wl} census PairPipeline.run ms: sgm {step_ms(sgm):.4f}  bp {step_ms(bp):.4f}", flush=True)
        del bp, sgm
    else:
        raise SystemExit(f"unknown item {what!r}")
    pipe = None
    torch.cuda.empty_cache()
