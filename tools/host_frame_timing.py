"""Per-call wall time of four host-frame calls with a given build of the library (profiles/host_frame_sim/README.md,
profiles/host_frame_refactor/README.md): a page-locked 352x288 4:2:0 frame (small direct path) and a registered 3840x2160 luma frame
(strips, results stored into the caller's plane), 200 calls after 20 warm-up calls each; a pageable 3840x2160 luma frame (strips, pushed
through the BAR where there is one, results through the ring), 100 calls after 20; and filter_sequence over 8 pageable 1920x1088 4:2:0
frames (the sequence's push transport), 40 calls after 5.  The process pins itself to the CPUs next to GPU 0 first.  One JSON line
is appended to OUT.

    python tools/host_frame_timing.py LIB LABEL OUT      # LIB: a libhevcdbk.so, of this commit or of another one
"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import _lib
_lib.LIB_PATH = sys.argv[1]
from gpu_video_codec_amd import deblock, shard, synth

# as bench.py: on the CPUs next to the GPU, before the first HIP call.  A process the scheduler puts on the far socket copies and polls
# across the socket link (0.35-0.40 ms against 0.31-0.33 ms for a pageable 4K luma frame), which is not what two libraries differ by
PINNED = shard.pin_to_gpu_cpus(0)

def per_call(fn, warm=20, n=200):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(n):
        a = time.perf_counter(); fn(); t.append(time.perf_counter() - a)
    t = np.array(t) * 1e6
    return {"median_us": float(np.median(t)), "mean_us": float(t.mean()), "min_us": float(t.min())}

out = {"label": sys.argv[2], "cpus_pinned": len(PINNED)}
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
    yp = synth.blocky_plane(3840, 2160, seed=6)
    out["pageable_4k_luma"] = per_call(lambda: ctx.filter_frame(yp, qp=32), n=100)
    seq = [synth.blocky_yuv420(1920, 1088, seed=10 + i) for i in range(8)]
    out["pageable_1080p_420_sequence_of_8"] = per_call(lambda: ctx.filter_sequence(seq, qp=32), warm=5, n=40)
print(json.dumps(out))
open(sys.argv[3], "a").write(json.dumps(out) + "\n")
