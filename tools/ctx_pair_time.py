"""Host time of the persistent context's synchronous pair call at a pipeline shape (dev tool, GPU box):
python tools/ctx_pair_time.py [workload] [pairs] [tag]
One context, three settings in turn: the defaults (smx_ctx_stereo_pair), colour guidance (smx_ctx_set_guidance +
smx_ctx_stereo_pair_rgb) and cross-based aggregation with Mei's parameters on the gray guide (smx_ctx_set_cross).  Per setting
3 warm-up pairs, then `pairs` timed ones: host clock around the call, which uploads the images, runs the pair, downloads the
six maps and synchronises.  Prints median / min / max in ms and a checksum of the six maps of the last pair, so that two builds
of the library can be compared (SMX_LIB_PATH with SMX_ALLOW_LIB_OVERRIDE=1 loads another build); `tag` leads every line.
The colour images of the synthetic pair are its gray images in three channels, (g, g // 2 + 60, 255 - g)."""
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import stereo_matching_cuda_amd as smx
from stereo_matching_cuda_amd import _lib, synth

wl = sys.argv[1] if len(sys.argv) > 1 else "kitti"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 12
tag = sys.argv[3] if len(sys.argv) > 3 else wl
L = smx.lib()
w, h, D = synth.SHAPES[wl]
dminl = -(D - 1)
gray = synth.gen_pair(w, h, D, synth.SEEDS.get(wl, 1))
rgb = [np.ascontiguousarray(np.stack((g, g // 2 + 60, 255 - g), axis=2).astype(np.uint8)) for g in gray]
names = ("best_l", "best_r", "dmap_l", "dmap_r", "occlusion", "filled")
bufs = {k: np.empty((h, w), np.float32) for k in names}
out = _lib.PairOut(**{k: v.ctypes.data for k, v in bufs.items()})
cross = smx.default_cross_params()
ctx = C.c_void_p()
_lib.check(L.smx_create(C.byref(smx.default_params()), w, h, D, C.byref(ctx)))


def pair(mode):
    if mode == "rgb":
        return L.smx_ctx_stereo_pair_rgb(ctx, rgb[0].ctypes.data, rgb[1].ctypes.data, 3, dminl, 0, C.byref(out))
    return L.smx_ctx_stereo_pair(ctx, gray[0].ctypes.data, gray[1].ctypes.data, dminl, 0, C.byref(out))


try:
    for mode in ("default", "rgb", "cross"):
        _lib.check(L.smx_ctx_set_guidance(ctx, 1 if mode == "rgb" else 0))
        _lib.check(L.smx_ctx_set_cross(ctx, C.byref(cross) if mode == "cross" else None))
        for _ in range(3):
            _lib.check(pair(mode))
        t = []
        for _ in range(N):
            t0 = time.perf_counter()
            rc = pair(mode)
            t.append((time.perf_counter() - t0) * 1e3)
            _lib.check(rc)
        sha = hashlib.sha1(b"".join(bufs[k].tobytes() for k in names)).hexdigest()[:16]
        print(f"{tag} {w}x{h}x{D} {mode:8s} median {np.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  pairs {N}  maps {sha}",
              flush=True)
finally:
    L.smx_destroy(ctx)
