"""Device time of the speckle filter (smx_dev_speckle_filter) at a pipeline shape (dev tool, GPU box):
python tools/speckle_time.py [workload] [repeats] [what ...]
what (default: pair constant random4 step):
  pair      the filter on the synthetic pair's own LR-checked map (PairPipeline, synth seed)
  constant  ... on a constant map: one component over every seam
  random4   ... on random integers over 4 labels at max_diff 0: many small components -- the extremes of component size
  step      PairPipeline.run with the filter on and off, alternating in this process
  on, off   PairPipeline.run of one pipeline only, a line per repeat.  `off` builds nothing of the feature, so it also
            runs against a checkout without it: `cd PARENT && python THIS/tools/speckle_time.py kitti 3 off`
            alternated with `on` in this tree compares the step with the filter on with the parent's default step.
Default parameters (max_size 200, max_diff 1) except random4.  A map prints one line: the rewritten pixels and, per repeat,
ms per call (host clock around 200 calls ended by a synchronise).
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/speckle_time.py kitti 1 MAP`,
one map and nothing else per run: the last 200 launches of each of k_speckle_tile, _seams, _sum, _apply are then the 200
timed calls (before them: one pipeline run and 20 warm-up calls), and `python tools/kernel_medians.py
DIR/*/*kernel_trace.csv k_speckle_ 200` reduces them."""
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
which = sys.argv[3:] or ["pair", "constant", "random4", "step"]
MAPS = ("pair", "constant", "random4")
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
need_on = any(k != "off" for k in which)
plain = PairPipeline(w, h, D)
on = PairPipeline(w, h, D, speckle=True) if need_on else None
plain.run(dl, dr)
if need_on:
    on.run(dl, dr)
torch.cuda.synchronize()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())
gen = torch.Generator(device="cuda").manual_seed(1)
maps = {"pair": (plain.occlusion, 1.0),
        "constant": (torch.full_like(plain.occlusion, float(plain.dminl + 3)), 1.0),
        "random4": (torch.randint(0, 4, (h, w), device="cuda", generator=gen).float() + plain.dminl, 0.0)}
out = torch.empty_like(plain.occlusion)
N = 200
for name in (k for k in which if k in MAPS):
    src, max_diff = maps[name]
    p = _lib.SpeckleParams()
    p.max_size, p.max_diff = 200, max_diff
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: smx.check(L.smx_dev_speckle_filter(C.byref(p), dp(src), dp(out), w, h, float(plain.dminl),
                                                      float(plain.dminl - 100), dp(on.speckle_ws), on.speckle_ws_bytes, st))
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    rewritten = int((out.view(torch.int32) != src.view(torch.int32)).sum())
    print(f"{wl} {w}x{h} map {name} max_size 200 max_diff {max_diff:g} rewritten {rewritten} ms/call "
          + " ".join(f"{v:.4f}" for v in ms), flush=True)


def step_ms(pipe):
    for _ in range(5):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        pipe.run(dl, dr)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 50 * 1e3


for what in which:
    for _ in range(reps if what in ("step", "on", "off") else 0):
        if what == "step":      # alternating, in one session
            print(f"{wl} PairPipeline.run ms: speckle off {step_ms(plain):.4f}  speckle on {step_ms(on):.4f}", flush=True)
        else:
            print(f"{wl} PairPipeline.run ms: speckle {what} {step_ms(on if what == 'on' else plain):.4f}", flush=True)
