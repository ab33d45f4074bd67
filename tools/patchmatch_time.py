"""Device time of PatchMatch stereo (smx_dev_patchmatch_pair, PairPipeline(aggregation="patchmatch")) at a pipeline shape (dev
tool, GPU box):  python tools/patchmatch_time.py [workload] [repeats] [what] [radius] [iterations]
what (default: step):
  search   smx_dev_patchmatch_pair on the synthetic pair of the workload's shape, radius (default 8) and iterations (default 4)
           as given, the other parameters at their defaults: 2 warm-up calls, then 5 back-to-back calls ended by a synchronise,
           ms per call by the host clock, a figure per repeat, and from it the window taps per second
  step     PairPipeline.run of the default pair and of aggregation="patchmatch" at radius 8 and 17 beside it, alternating inside
           each repeat, 3 calls each
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/patchmatch_time.py kitti 1 search`, one
`what` and nothing else per run; then `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_pm 5`."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
what = sys.argv[3] if len(sys.argv) > 3 else "step"
radius = int(sys.argv[4]) if len(sys.argv) > 4 else 8
iterations = int(sys.argv[5]) if len(sys.argv) > 5 else 4

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()


def timed(call, warm, n):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def pm_pipe(r, it):
    p = smx.default_pm_params()
    p.radius, p.iterations = r, it
    return PairPipeline(w, h, D, aggregation="patchmatch", pm_params=p)


def window_sums(it):
    """plane-cost evaluations per pixel and view: the initialisation, and per iteration 8 spatial candidates, the refinement
    steps and the view candidate"""
    k, dd = 0, (D - 1) * 0.5
    while dd >= 0.1:
        k, dd = k + 1, dd * 0.5
    return 1 + it * (8 + k + 1), k


if what == "search":
    pipe = pm_pipe(radius, iterations)
    ms = [timed(lambda: pipe.aggregate(dl, dr), 2, 5) for _ in range(reps)]
    sums, k = window_sums(iterations)
    taps = 2 * w * h * sums * (2 * radius + 1) ** 2          # (an upper bound: the windows at the border are clipped)
    print(f"{wl} {w}x{h}xD{D} radius {radius} iterations {iterations} ({k} refinement steps, {sums} window sums a pixel and view, "
          f"{taps} taps): smx_dev_patchmatch_pair ms/call " + " ".join(f"{v:.3f}" for v in ms) +
          f"; {taps / min(ms) / 1e6:.1f} G taps/s at the best", flush=True)
else:
    pipes = {"default pair": PairPipeline(w, h, D), "patchmatch r8": pm_pipe(8, iterations), "patchmatch r17": pm_pipe(17, iterations)}
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} PairPipeline.run ms: " + "  ".join(f"{k} {timed(lambda: q.run(dl, dr), 1, 3):.4f}" for k, q in pipes.items()),
              flush=True)
    for q in pipes.values():
        q.check_status()
