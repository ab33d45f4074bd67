"""Device time of the weighted-median refinement (smx_dev_weighted_median) at a pipeline shape (dev tool, GPU box):
python tools/wmf_time.py [workload] [repeats]
The maps are the synthetic pair's own filled / occlusion maps (PairPipeline, synth seed); radius 9, default sigmas.
Prints one line per mode: ms per call (host clock around N calls ended by a synchronise) and the selected pixels.
Kernel times: run it under `rocprofv3 --kernel-trace --stats` (kernel k_weighted_median)."""
import ctypes as C
import sys
import time

import torch

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
pipe = PairPipeline(w, h, D)
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
pipe.run(dl, dr)
out = torch.empty_like(pipe.filled)
p = smx.default_wmf_params()
L = smx.lib()
dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
selected = int((pipe.occlusion.trunc() < pipe.dminl).sum())
N = 200
for mode, sel in (("all", None), ("occluded", pipe.occlusion)):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: smx.check(L.smx_dev_weighted_median(C.byref(p), dp(dl), dp(pipe.filled), dp(sel), dp(out), w, h,
                                                       pipe.dminl, D, st))
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
    print(f"{wl} {w}x{h} D={D} radius {p.radius} mode {mode} selected {w * h if sel is None else selected} "
          f"ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)
