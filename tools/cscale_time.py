"""Device time of cross-scale aggregation (smx_dev_cscale_wta_pair, PairPipeline(cross_scale=...)) at a pipeline shape (dev tool,
GPU box):  python tools/cscale_time.py [workload] [repeats] [what] [scales]
what (default: step):
  none, inplace   smx_dev_cscale_wta_pair on both views of the workload's shape, `scales` levels (default 4), lambda 1.0, random
                  volumes; `none` stores no combined volume, `inplace` stores it over level 0: 10 warm-up calls, then 100
                  back-to-back calls ended by a synchronise, ms per call by the host clock, a figure per repeat
  wta             the yardstick: PairPipeline(want_agg=True).run on the synthetic pair, 10 + 100 times -- its trace holds the
                  natural-order winner-take-all pass over the materialised volumes of the same shape (k_wta<Natural, ..>)
  step            PairPipeline.run with adjust=True (the configuration that also keeps the volumes) and with cross_scale of 2 and
                  4 scales beside it, alternating inside each repeat, 20 calls each
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cscale_time.py kitti 1 inplace 4`, one
`what` and nothing else per run; then `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_cscale 100` (k_wta for `wta`)."""
import ctypes as C
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import _lib, synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
what = sys.argv[3] if len(sys.argv) > 3 else "step"
scales = int(sys.argv[4]) if len(sys.argv) > 4 else 4
WARM, N = 10, 100

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
L = smx.lib()
BIG = dict(max_ws_bytes=16 << 30)
dminl = -(D - 1)


def timed(call, n):
    for _ in range(WARM if n == N else 3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


if what in ("none", "inplace"):
    p = smx.default_cscale_params()
    p.scales = scales
    g = torch.Generator(device="cuda").manual_seed(1)
    vols, cells = [], 0
    for dmin in (dminl, 0):
        view = []
        for s in range(scales):
            ws, hs, _, ds = _lib.cscale_level(w, h, dmin, D, s)
            view.append(torch.randn((ds, hs, ws), device="cuda", generator=g) if s else None)
            cells += ds * hs * ws
        vols.append(view)
    lv0 = torch.randn((2, D, h, w), device="cuda", generator=g)
    keys = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    arrays = [(C.c_void_p * scales)(*([lv0[v].data_ptr()] + [t.data_ptr() for t in vols[v][1:]])) for v in range(2)]
    out = C.c_void_p(lv0.data_ptr()) if what == "inplace" else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: smx.check(L.smx_dev_cscale_wta_pair(C.byref(p), arrays[0], arrays[1], w, h, dminl, 0, D, C.c_void_p(keys.data_ptr()),
                                                       out, None, None, st))
    ms = [timed(call, N) for _ in range(reps)]
    read, wrote = 4 * cells, (8 * D * w * h if out else 0) + 16 * w * h
    print(f"{wl} {w}x{h}x{D} scales {scales} out {what}: reads {read} bytes (level 0 alone {8 * D * w * h}), writes {wrote}; "
          f"smx_dev_cscale_wta_pair ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)
elif what == "wta":
    pipe = PairPipeline(w, h, D, want_agg=True, **BIG)
    ms = [timed(lambda: pipe.run(dl, dr), N) for _ in range(reps)]
    print(f"{wl} {w}x{h}x{D} PairPipeline(want_agg=True).run ms " + " ".join(f"{v:.4f}" for v in ms), flush=True)
else:
    pipes = {"adjust": PairPipeline(w, h, D, adjust=True, **BIG)}
    for s in (2, 4):
        p = smx.default_cscale_params()
        p.scales = s
        pipes[f"cross-scale {s}"] = PairPipeline(w, h, D, cross_scale=p, **BIG)
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} PairPipeline.run ms: " + "  ".join(f"{k} {timed(lambda: q.run(dl, dr), 20):.4f}" for k, q in pipes.items()),
              flush=True)
    for k, q in pipes.items():
        q.check_status()
    a, b = pipes["adjust"].dmap[0], pipes["cross-scale 4"].dmap[0]
    print(f"{wl} left winners that differ between the plain and the 4-scale pair: {int((a != b).sum())} of {w * h}", flush=True)
