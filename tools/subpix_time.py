"""Cost of the sub-pixel refinement per pair step at a pipeline shape (dev tool, GPU box):
python tools/subpix_time.py [workload] [repeats]
Two PairPipelines on the synthetic pair, one plain and one with subpixel="parabola", in one process; each repeat times N
steps of one, then N of the other (alternating, so that clocks and caches drift alike for both).  Prints ms per pair step
(aggregate + finish, + smx_dev_subpixel_pair for the sub-pixel one; host clock around N steps ended by a synchronise).
Kernel times: run it under `rocprofv3 --kernel-trace --stats` (k_wta<Comb, 4, false> against k_wta<Comb, 4, true>, k_subpixel_pair)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
pipes = {"plain": PairPipeline(w, h, D), "subpixel": PairPipeline(w, h, D, subpixel="parabola")}
N = 50
for p in pipes.values():
    for _ in range(10):
        p.run(dl, dr)
    p.check_status()
ms = {k: [] for k in pipes}
for _ in range(reps):
    for k, p in pipes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            p.run(dl, dr)
        torch.cuda.synchronize()
        ms[k].append((time.perf_counter() - t0) / N * 1e3)
for k in pipes:
    pipes[k].check_status()
    print(f"{wl} {w}x{h} D={D} {k:8s} ms/pair " + " ".join(f"{v:.4f}" for v in ms[k]), flush=True)
a, b = sorted(ms["plain"])[reps // 2], sorted(ms["subpixel"])[reps // 2]
print(f"median: plain {a:.4f} ms, subpixel {b:.4f} ms, {100 * (b - a) / a:+.2f} %", flush=True)
