"""Per-call wall time of two host-frame calls with a given build of the library (profiles/host_frame_sim/README.md):
a page-locked 352x288 4:2:0 frame (small direct path) and a registered 3840x2160 luma frame (strips, results stored into the caller's
plane), 200 calls after 20 warm-up calls each.  One JSON line is appended to OUT.

    python tools/host_frame_timing.py LIB LABEL OUT      # LIB: a libhevcdbk.so, of this commit or of another one
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import _lib
_lib.LIB_PATH = sys.argv[1]
from gpu_video_codec_amd import deblock, synth

def per_call(fn, warm=20, n=200):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        a = time.perf_counter(); fn(); t.append(time.perf_counter() - a)
    t = np.array(t) * 1e6
    return {"median_us": float(np.median(t)), "mean_us": float(t.mean()), "min_us": float(t.min())}

out = {"label": sys.argv[2]}
with deblock.Context(0) as ctx:
    y, u, v = synth.blocky_yuv420(352, 288, seed=3)
    pl = [ctx.pinned_array(p.shape) for p in (y, u, v)]
    for a, b in zip(pl, (y, u, v)):
        a[:] = b
    out["pinned_cif_420"] = per_call(lambda: ctx.filter_frame(*pl, qp=35))
    for a in pl:
        ctx.free_pinned(a)
    y4 = synth.blocky_plane(3840, 2160, seed=5)
    ctx.host_register(y4)
    out["registered_4k_luma"] = per_call(lambda: ctx.filter_frame(y4, qp=32))
    ctx.host_unregister(y4)
print(json.dumps(out))
open(sys.argv[3], "a").write(json.dumps(out) + "\n")
