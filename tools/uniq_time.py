"""Device time of the uniqueness filter at a pipeline shape (dev tool, GPU box):
python tools/uniq_time.py [workload] [repeats] [what ...]
what (default: step):
  step      PairPipeline.run with uniqueness=0.25 against the default pipeline, alternating in this process: ms per pair step
            (host clock around 50 back-to-back steps ended by a synchronise), a line per repeat, the medians last
  on, off   PairPipeline.run of one pipeline only, a line per repeat
  nbr_on, nbr_off   the same with subpixel="parabola" (the nbr+uq / nbr forms of the WTA pass)
  filter    smx_dev_uniqueness alone on the state of one run: ms per call over 200 back-to-back calls
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/uniq_time.py kitti 1 on` (then
`off`), one `what` and nothing else per run; `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_wta 50` reduces the WTA
pass of the last 50 steps."""
import ctypes as C
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
which = sys.argv[3:] or ["step"]
RATIO = 0.25
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
on = PairPipeline(w, h, D, uniqueness=RATIO) if any(k in ("step", "on", "filter") for k in which) else None
off = PairPipeline(w, h, D) if any(k in ("step", "off") for k in which) else None
nbr_on = PairPipeline(w, h, D, uniqueness=RATIO, subpixel="parabola") if "nbr_on" in which else None
nbr_off = PairPipeline(w, h, D, subpixel="parabola") if "nbr_off" in which else None
PIPES = {"on": on, "off": off, "nbr_on": nbr_on, "nbr_off": nbr_off}
for pipe in PIPES.values():
    if pipe is not None:
        pipe.run(dl, dr)
torch.cuda.synchronize()


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
    if what == "filter":
        L, dp = smx.lib(), lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda: smx.check(L.smx_dev_uniqueness(RATIO, dp(on.keys[0]), dp(on.uq[0]), dp(on.occlusion), dp(on.unique),
                                                      dp(on.margin), w, h, float(on.dminl), float(on.dminl - 100), st))
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(200):
                call()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / 200 * 1e3)
        print(f"{wl} {w}x{h} smx_dev_uniqueness ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)
        continue
    a, b = [], []
    for _ in range(reps):
        if what == "step":      # alternating, in one session
            a.append(step_ms(off))
            b.append(step_ms(on))
            print(f"{wl} PairPipeline.run ms: off {a[-1]:.4f}  on {b[-1]:.4f}", flush=True)
        else:
            print(f"{wl} PairPipeline.run ms: {what} {step_ms(PIPES[what]):.4f}", flush=True)
    if a:
        print(f"{wl} PairPipeline.run median ms: off {statistics.median(a):.4f}  on {statistics.median(b):.4f}  "
              f"(+{(statistics.median(b) / statistics.median(a) - 1) * 100:.2f} %)", flush=True)
