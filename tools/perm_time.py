"""Device time of the permeability filter (smx_dev_permeability_wta_pair, PairPipeline(permeability=...)) at a pipeline shape
(dev tool, GPU box):  python tools/perm_time.py [workload] [repeats] [what]
what (default: step):
  filter    smx_dev_permeability_wta_pair on both views of the workload's shape, random volumes, sigma 32, the guide the
            synthetic pair's gray images, a workspace for every slice at once up to 1 GiB (what the context takes): 10 warm-up
            calls, then 100 back-to-back calls ended by a synchronise, ms per call by the host clock, a figure per repeat.  The
            filtered volumes go to a buffer of their own, so that every call filters the same values (in place they would grow
            from call to call); the bytes moved are those of the in-place call: the horizontal pass reads one buffer and writes
            the other, the vertical pass runs in place either way
  wta       the first yardstick: PairPipeline(want_agg=True).run on the synthetic pair, 10 + 100 times -- its trace holds the
            natural-order winner-take-all pass over the materialised volumes of the same shape (k_wta<Natural, ..>)
  cscale    the second yardstick: smx_dev_cscale_wta_pair in place at 2 scales on random volumes (k_cscale), 10 + 100 times
  step      PairPipeline.run with adjust=True (the configuration that also keeps the volumes) and with permeability=True beside
            it, alternating inside each repeat, 20 calls each; then the left winners that differ
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/perm_time.py kitti 1 filter`, one
`what` and nothing else per run; then `python tools/kernel_medians.py DIR/*/*kernel_trace.csv k_perm_h 100` (k_perm_v,
k_perm_weights; k_wta for `wta`, k_cscale for `cscale`)."""
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
WARM, N = 10, 100

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
L = smx.lib()
BIG = dict(max_ws_bytes=16 << 30)
dminl = -(D - 1)
vp = lambda t: C.c_void_p(t.data_ptr())


def timed(call, n):
    for _ in range(WARM if n == N else 3):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


if what == "filter":
    p = smx.default_perm_params()
    g = torch.Generator(device="cuda").manual_seed(1)
    vol = torch.randn((2, D, h, w), device="cuda", generator=g)
    out = torch.empty_like(vol)
    keys = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    per = 2 * w * h * 4
    chunk = min(D, max(1, (1 << 30) // per - 2))
    ws = torch.empty(per * (2 + chunk), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        smx.check(L.smx_dev_permeability_wta_pair(C.byref(p), vp(vol[0]), vp(vol[1]), vp(dl), vp(dr), 1, w, h, dminl, 0, D, vp(keys),
                                                  vp(out), None, None, vp(ws), ws.numel(), st))

    ms = [timed(call, N) for _ in range(reps)]
    v = 8 * D * w * h
    print(f"{wl} {w}x{h}x{D} {chunk} slices a chunk ({-(-D // chunk)} chunks), workspace {ws.numel()} bytes: each pass "
          f"reads the volumes twice ({2 * v} bytes) and the scratch once ({v}), writes the scratch and the volumes ({2 * v}); the "
          f"winner-take-all pass reads {v}; smx_dev_permeability_wta_pair ms/call " + " ".join(f"{x:.4f}" for x in ms), flush=True)
elif what == "wta":
    pipe = PairPipeline(w, h, D, want_agg=True, **BIG)
    ms = [timed(lambda: pipe.run(dl, dr), N) for _ in range(reps)]
    print(f"{wl} {w}x{h}x{D} PairPipeline(want_agg=True).run ms " + " ".join(f"{v:.4f}" for v in ms), flush=True)
elif what == "cscale":
    p = smx.default_cscale_params()
    p.scales = 2
    g = torch.Generator(device="cuda").manual_seed(1)
    lv0 = torch.randn((2, D, h, w), device="cuda", generator=g)
    lv1 = []
    for dmin in (dminl, 0):
        ws_, hs_, _, ds_ = _lib.cscale_level(w, h, dmin, D, 1)
        lv1.append(torch.randn((ds_, hs_, ws_), device="cuda", generator=g))
    keys = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    arrays = [(C.c_void_p * 2)(lv0[v].data_ptr(), lv1[v].data_ptr()) for v in range(2)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda: smx.check(L.smx_dev_cscale_wta_pair(C.byref(p), arrays[0], arrays[1], w, h, dminl, 0, D, vp(keys), vp(lv0), None,
                                                       None, st))
    ms = [timed(call, N) for _ in range(reps)]
    print(f"{wl} {w}x{h}x{D} smx_dev_cscale_wta_pair in place, 2 scales, ms/call " + " ".join(f"{v:.4f}" for v in ms), flush=True)
else:
    pipes = {"adjust": PairPipeline(w, h, D, adjust=True, **BIG), "permeability": PairPipeline(w, h, D, permeability=True, **BIG)}
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} PairPipeline.run ms: " + "  ".join(f"{k} {timed(lambda: q.run(dl, dr), 20):.4f}" for k, q in pipes.items()),
              flush=True)
    for k, q in pipes.items():
        q.check_status()
    plain = PairPipeline(w, h, D, want_agg=True, **BIG)
    plain.run(dl, dr)
    a, b = plain.dmap[0], pipes["permeability"].dmap[0]
    print(f"{wl} left winners that differ between the plain and the filtered pair: {int((a != b).sum())} of {w * h}", flush=True)
