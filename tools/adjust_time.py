"""Device time of the depth-discontinuity adjustment (smx_dev_discontinuity_adjust) at a pipeline shape (dev tool, GPU box):
python tools/adjust_time.py [workload] [repeats] [what ...]
The map is the one the stage meets: the filled left map of PairPipeline(cost="census", aggregation="sgm") on the synthetic pair of
the workload, with that pipeline's left aggregated volume.  The shares of pixels that have a candidate and that change are counted
with tests/adjust_ref.py and printed.
what (default: call step):
  call          smx_dev_discontinuity_adjust with the default parameters (one round, one launch) on that map, out of place: 10
                warm-up calls, then 100 back-to-back calls ended by a synchronise, ms per call by the host clock, a figure per
                repeat
  step          PairPipeline.run with and without adjust=True, alternating inside each repeat, 20 calls each, for
                aggregation="sgm" (census cost) and for the guided default; for the guided default also without the adjustment
                but with the volumes kept (want_agg=True): what keeping them costs that path
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/adjust_time.py kitti 1 call`, one
`what` and nothing else per run; then `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_adjust_round 100`."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import adjust_ref  # noqa: E402
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["call", "step"]
WARM, N = 10, 100

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())
BIG = dict(max_ws_bytes=16 << 30)

if "call" in which:
    x = PairPipeline(w, h, D, cost="census", aggregation="sgm", adjust=True, **BIG)
    x.aggregate(dl, dr)
    x.adjust, keep = None, x.adjust             # the filled map in front of the stage
    x.finish()
    torch.cuda.synchronize()
    x.adjust = keep
    filled, vol = x.filled.clone(), x.agg[0]
    stats = {}
    want = adjust_ref.adjust(filled.cpu().numpy(), vol.cpu().numpy(), x.dminl, stats=stats, **adjust_ref.DEFAULTS)
    n = w * h
    cand, changed = stats["changed"] + stats["unchanged"], stats["changed"]
    gathers = cand + stats["candidate_h"] + stats["candidate_v"]           # at least: the own cost and one per axis with a candidate
    print(f"{wl} {w}x{h}x{D}: {cand} of {n} pixels have a candidate ({100.0 * cand / n:.2f} %), {changed} change "
          f"({100.0 * changed / n:.2f} %); map read + written {8 * n} bytes a round, gathers at least {4 * gathers} bytes "
          f"(32-byte sectors: {32 * gathers}); workspace {x.adjust_ws_bytes / 2**20:.1f} MiB, volume {vol.numel() * 4 / 2**30:.3f} GiB",
          flush=True)
    P = smx.default_adjust_params()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(filled)
    call = lambda: smx.check(L.smx_dev_discontinuity_adjust(C.byref(P), dp(filled), dp(vol), dp(out), w, h, x.dminl, D, 0, None,
                                                            dp(x.adjust_ws), x.adjust_ws_bytes, st))
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    print(f"{wl} {w}x{h}x{D} tau_e {P.tau_e} vertical {P.vertical} iterations {P.iterations} smx_dev_discontinuity_adjust ms/call "
          + " ".join(f"{v:.4f}" for v in ms), flush=True)
    del x, filled, vol, out


def step_ms(pipe):
    run = lambda: pipe.run(dl, dr)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3


if "step" in which:
    for name, kw in (("census + sgm", dict(cost="census", aggregation="sgm")), ("guided default", {})):
        pipes = {"off": PairPipeline(w, h, D, **kw, **BIG), "adjust": PairPipeline(w, h, D, adjust=True, **kw, **BIG)}
        if not kw:
            pipes["off, volumes kept"] = PairPipeline(w, h, D, want_agg=True, **BIG)
        for _ in range(reps):       # alternating, in one session
            print(f"{wl} PairPipeline.run {name} ms: " + "  ".join(f"{k} {step_ms(p):.4f}" for k, p in pipes.items()), flush=True)
        del pipes
