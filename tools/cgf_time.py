"""Device time of the colour-guided filter aggregation (smx_dev_cgf_wta_pair) at a pipeline shape (dev tool, GPU box):
python tools/cgf_time.py [workload] [repeats] [what ...]
what (default: call step):
  call          the whole smx_dev_cgf_wta_pair call on the reference cost volumes of the synthetic pair, both views, with the
                aggregated volumes and the states off, every slice the workspace bound admits in flight: ms per call (host
                clock around 20 back-to-back calls ended by a synchronise), a figure per repeat
  step          PairPipeline.run: guidance="rgb" against the gray multi-kernel path (multi_kernel=True, smx_set_agg_path(1)) and
                the default gray path, alternating in this process
  rgb, gray_mk  PairPipeline.run of one pipeline only, a line per repeat
The colour guide of the synthetic pair is its gray image in three channels, (g, g // 2 + 60, 255 - g): the times do not
depend on the values.
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cgf_time.py kitti 1 call`, one
`what` and nothing else per run; `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_cgf_ 20` reduces the launches of
the 20 timed calls."""
import ctypes as C
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["call", "step"]
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
colour = lambda g: np.ascontiguousarray(np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
cl, cr = torch.from_numpy(colour(Il)).cuda(), torch.from_numpy(colour(Ir)).cuda()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())
need_rgb = any(k in ("call", "step", "rgb") for k in which)
need_gray = any(k in ("step", "gray_mk") for k in which)
rgb = PairPipeline(w, h, D, guidance="rgb", max_ws_bytes=16 << 30) if need_rgb else None
gray_mk = PairPipeline(w, h, D, multi_kernel=True, max_ws_bytes=16 << 30) if need_gray else None
gray = PairPipeline(w, h, D) if "step" in which else None


def run(pipe):
    if pipe is rgb:
        pipe.run(dl, dr, rgb_l=cl, rgb_r=cr)
    elif pipe is gray_mk:
        smx.check(L.smx_set_agg_path(1))
        try:
            pipe.run(dl, dr)
        finally:
            L.smx_set_agg_path(0)
    else:
        pipe.run(dl, dr)


for pipe in (rgb, gray_mk, gray):
    if pipe is not None:
        run(pipe)
torch.cuda.synchronize()
if rgb is not None:
    print(f"{wl} {w}x{h}x{D} guidance=rgb: {rgb.slices_in_flight} slices in flight, workspace {rgb.cgf_ws_bytes / 2**20:.0f} MiB",
          flush=True)
if gray_mk is not None:
    print(f"{wl} gray multi-kernel: {gray_mk.slices_in_flight} slices in flight, workspace {gray_mk.ws_bytes / 2**20:.0f} MiB",
          flush=True)

N = 20
if "call" in which:
    cost_l, cost_r = rgb.cost_volumes(dl, dr)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = smx.default_params()
    call = lambda: smx.check(L.smx_dev_cgf_wta_pair(C.byref(P), dp(cl), dp(cr), 3, dp(cost_l), dp(cost_r), w, h, 0, D,
                                                    dp(rgb.keys), None, None, None, dp(rgb.cgf_ws), rgb.cgf_ws_bytes, st))
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            call()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    print(f"{wl} {w}x{h}x{D} smx_dev_cgf_wta_pair radius {P.radius} ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)


def step_ms(pipe):
    for _ in range(3):
        run(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(N):
        run(pipe)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / N * 1e3


for what in which:
    for _ in range(reps if what in ("step", "rgb", "gray_mk") else 0):
        if what == "step":      # alternating, in one session
            print(f"{wl} PairPipeline.run ms: gray default {step_ms(gray):.4f}  gray multi-kernel {step_ms(gray_mk):.4f}  "
                  f"rgb {step_ms(rgb):.4f}", flush=True)
        else:
            print(f"{wl} PairPipeline.run ms: {what} {step_ms(rgb if what == 'rgb' else gray_mk):.4f}", flush=True)
