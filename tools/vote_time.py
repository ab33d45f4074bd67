"""Device time of region voting (smx_dev_cross_arms on the left guide + smx_dev_region_vote) at a pipeline shape (dev tool, GPU
box):  python tools/vote_time.py [workload] [repeats] [what ...]
The map is the one the stage meets: the left map of PairPipeline(cost="adcensus", aggregation="cross", uniqueness=UNIQ %,
speckle=True) on the synthetic pair of tools/cross_time.py, behind LR check, uniqueness and speckle removal; its outliers are
counted and printed.  UNIQ is 0.5: the AD-Census margins of the synthetic pair are narrow, and from 5 % on the uniqueness test
leaves no valid pixel at all (every pixel an outlier without a voter in reach: the stage's worst case, not its use).
what (default: call step):
  call          one arms launch and one smx_dev_region_vote call with the default parameters on that map: 10 warm-up calls, then
                ms per call (host clock around 30 back-to-back calls ended by a synchronise), a figure per repeat; the same for
                smx_dev_region_vote alone
  step          PairPipeline.run with and without vote=True, alternating inside each repeat
  trace CSV     no GPU: reduces the kernel trace of a `call` run with repeats = 1.  A call is a fixed sequence of launches (the
                arms, one per round, the interpolation), so the launches are reduced by their position in the call: median,
                minimum and maximum over the last 30 calls, in microseconds
Kernel times: `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vote_time.py kitti 1 call`, one
`what` and nothing else per run; then `python tools/vote_time.py kitti 1 trace DIR/*/*kernel_trace.csv`."""
import ctypes as C
import sys
import time

import numpy as np

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
which = sys.argv[3:] or ["call", "step"]
WARM, N = 10, 30
UNIQ = 0.5

if which[0] == "trace":
    import csv
    import statistics
    rows = []
    with open(which[1], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_vote_" in name or "k_cross_arms" in name:
                short = name.replace("(anonymous namespace)::", "").replace("smx::", "").removeprefix("void ").split("(")[0]
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short))
    rows.sort()
    # a call: an arms launch with voting kernels right behind it, up to the next arms launch
    starts = [i for i, r in enumerate(rows[:-1]) if "k_cross_arms" in r[2] and "k_vote_" in rows[i + 1][2]]
    ends = starts[1:] + [len(rows)]
    calls = [rows[a:b] for a, b in zip(starts, ends)]
    per = len(calls[-1])
    calls = [c for c in calls if len(c) == per][-N:]
    print(f"{len(starts)} calls of {per} launches, the last {len(calls)} taken")
    total = 0.0
    for k in range(per):
        us = [(c[k][1] - c[k][0]) / 1e3 for c in calls]
        total += statistics.median(us)
        print(f"  {k:2d} {calls[0][k][2]:<24} median {statistics.median(us):9.2f} min {min(us):9.2f} max {max(us):9.2f}")
    print(f"sum of medians {total:.2f}")
    sys.exit(0)

import torch  # noqa: E402

sys.path.insert(0, ".")
import stereo_matching_cuda_amd as smx  # noqa: E402
from stereo_matching_cuda_amd import synth  # noqa: E402
from stereo_matching_cuda_amd.device import PairPipeline  # noqa: E402

w, h, D = synth.SHAPES[wl]
Il, Ir = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
colour = lambda g: np.ascontiguousarray(np.stack([g, g // 2 + 60, 255 - g], axis=-1).astype(np.uint8))
dl, dr = torch.from_numpy(Il).cuda(), torch.from_numpy(Ir).cuda()
cl, cr = torch.from_numpy(colour(Il)).cuda(), torch.from_numpy(colour(Ir)).cuda()
L = smx.lib()
dp = lambda t: C.c_void_p(t.data_ptr())

kw = dict(cost="adcensus", aggregation="cross", uniqueness=UNIQ / (100.0 - UNIQ), speckle=True, max_ws_bytes=16 << 30)
pipes = {"off": PairPipeline(w, h, D, **kw), "vote": PairPipeline(w, h, D, vote=True, **kw)}
for p in pipes.values():
    p.run(dl, dr, rgb_l=cl, rgb_r=cr)
torch.cuda.synchronize()
x = pipes["vote"]
kept = x.despeckled.clone()
dmin = x.dminl
k = kept.cpu().numpy()
valid = np.isfinite(k) & (np.trunc(np.where(np.isfinite(k), k, 0)) >= dmin)
left = x.voted.cpu().numpy()
still = ~(np.isfinite(left) & (np.trunc(np.where(np.isfinite(left), left, 0)) >= dmin))
print(f"{wl} {w}x{h}x{D}: {int((~valid).sum())} outliers of {valid.size} pixels ({100.0 * (~valid).mean():.1f} %) behind LR check, "
      f"uniqueness {UNIQ} % and speckle removal; {int(still.sum())} left behind voting and interpolation; workspace "
      f"{x.vote_ws_bytes / 2**20:.1f} MiB", flush=True)


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(N):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / N * 1e3)
    return " ".join(f"{v:.4f}" for v in ms)


if "call" in which:
    V, A = smx.default_vote_params(), smx.default_cross_params()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty_like(kept)
    arms = lambda: smx.check(L.smx_dev_cross_arms(C.byref(A), dp(cl), None, 3, w, h, dp(x.vote_arms_plane), st))
    vote = lambda: smx.check(L.smx_dev_region_vote(C.byref(V), dp(x.vote_arms_plane), dp(cl), 3, dp(kept), dp(x.dmap[1]), dp(out), w, h,
                                                   dmin, D, int(x.params.d_lr), dp(x.vote_ws), x.vote_ws_bytes, st))

    def both():
        arms()
        vote()

    head = f"{wl} {w}x{h}x{D} tau_s {V.tau_s} tau_h_pct {V.tau_h_pct} iterations {V.iterations} interpolate {V.interpolate}"
    print(f"{head} arms + smx_dev_region_vote ms/call {timed(both)}", flush=True)
    if reps > 1:        # (a profiled run keeps to the one sequence of launches)
        print(f"{head} smx_dev_region_vote ms/call {timed(vote)}", flush=True)


def step_ms(name):
    run = lambda: pipes[name].run(dl, dr, rgb_l=cl, rgb_r=cr)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 20 * 1e3


if "step" in which:
    for _ in range(reps):       # alternating, in one session
        print(f"{wl} PairPipeline.run adcensus + cross + uniqueness + speckle ms: " +
              "  ".join(f"{name} {step_ms(name):.4f}" for name in pipes), flush=True)
