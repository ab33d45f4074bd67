"""Device time of semi-global matching (smx_dev_sgm_wta_pair) at a pipeline shape (dev tool, GPU box):
python tools/sgm_time.py [workload] [repeats] [what ...]
what (default: call4 call8 step):
  call4, call8  the whole smx_dev_sgm_wta_pair call on the synthetic pair's census volumes, both views, paths 4 / 8, with
                the S volumes and the neighbour state off: ms per call (host clock around 200 back-to-back calls ended by
                a synchronise), a figure per repeat
  step          PairPipeline.run with cost="census": aggregation="sgm" (paths 8) against the guided filter, alternating in
                this process
  sgm, guided   PairPipeline.run of one pipeline only, a line per repeat.  `guided` is tools/census_time.py's census step,
                so against a checkout without the feature run that tool there and alternate it with `sgm` here.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/sgm_time.py kitti 1 call8`, one
`what` and nothing else per run: the last 200 launches of each kernel are the 200 timed calls (k_sgm_cols: the last 400 /
1200, two / six launches a call), and `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_sgm_ 200` reduces them."""
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
which = sys.argv[3:] or ["call4", "call8", "step"]
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
need_sgm = any(k != "guided" for k in which)
need_guided = any(k in ("step", "guided") for k in which)
sgm = PairPipeline(w, h, D, cost="census", aggregation="sgm") if need_sgm else None
guided = PairPipeline(w, h, D, cost="census") if need_guided else None
for pipe in (sgm, guided):
    if pipe is not None:
        pipe.run(dl, dr)
torch.cuda.synchronize()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())
N = 200
for name in (k for k in which if k in ("call4", "call8")):
    p = _lib.default_sgm_params()
    p.paths = 4 if name == "call4" else 8
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: smx.check(L.smx_dev_sgm_wta_pair(C.byref(p), dp(sgm.sgm_cost[0]), dp(sgm.sgm_cost[1]), w, h, D,
                                                    dp(sgm.keys), None, None, dp(sgm.sgm_ws), sgm.sgm_ws_bytes, st))
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
    print(f"{wl} {w}x{h}x{D} smx_dev_sgm_wta_pair paths {p.paths} p1 {p.p1} p2 {p.p2} ms/call "
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
    for _ in range(reps if what in ("step", "sgm", "guided") else 0):
        if what == "step":      # alternating, in one session
            print(f"{wl} census PairPipeline.run ms: guided {step_ms(guided):.4f}  sgm {step_ms(sgm):.4f}", flush=True)
        else:
            print(f"{wl} census PairPipeline.run ms: {what} {step_ms(sgm if what == 'sgm' else guided):.4f}", flush=True)
