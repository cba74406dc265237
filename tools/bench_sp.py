#!/usr/bin/env python3
"""Same-process A/B for semi-planar chroma (the _sp entry): what the Cb / Cr pairs of a 4:2:0 picture cost in ONE launch on the
interleaved plane against what a caller had before -- two launches of the planar _g4 entries on the split planes -- through another
build (the parent commit's libhevcdbk.so) and through this one (whose planar entries must not have moved).

    python3 tools/bench_sp.py parent/libhevcdbk.so [--lib gpu_video_codec_amd/libhevcdbk.so] [--bit-depth 8 --bit-depth 10]

Both libraries are loaded into ONE process (ctypes, RTLD_LOCAL), work on the same device buffers and take turns
  a parent_planar   b this_planar   c this_sp   a parent_planar_again
per round (the order reversed every other round): each turn 20 untimed calls, then --steps back-to-back calls between two events
recorded on the library's own stream, after 150 settling calls of every variant.  `median_ms` is the time BETWEEN THE EVENTS per call
-- what the stream spent, not what the host spent enqueueing: (a) makes two launches per call and (c) one, and the wall clock around
the same calls (`wall_ms`, one synchronisation at the end) is reported beside it so that the two can be told apart.  Reported per
workload: the median over --rounds of every variant and `spread_ms` = |median(a) - median(a again)|, the run-to-run spread of the
yardstick; the expectation under test is c <= a + spread.
The split and merge passes a caller of (a) needs are NOT in (a); --passes times them (tools/ubench/sp_passes: 16 bytes of the pair
plane per lane) beside a plain copy of the same bytes.
Workloads: the pair planes of 1920x1080 (960x540) and 3840x2160 (1920x1080), --frames frames per call, bS 2 on every interior edge;
  deblock  the packed deblocking kernels, src -> dst, one QP and a QP map per 16x16 luma samples
One JSON line per workload and bit depth."""
import argparse, ctypes as C, json, os, subprocess, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_video_codec_amd import _lib as L0, synth  # struct definitions only  # noqa: E402
from bench_g4 import VP, Pool  # noqa: E402


class Lib:
    def __init__(self, path):
        self.path = os.path.abspath(path)
        L = self.L = C.CDLL(self.path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        L.hevcdbk_create.argtypes = [C.c_int, C.POINTER(VP)]
        L.hevcdbk_destroy.argtypes = [VP]
        L.hevcdbk_device_malloc.argtypes = [VP, C.c_size_t, C.POINTER(VP)]
        L.hevcdbk_memcpy_h2d.argtypes = [VP, VP, VP, C.c_size_t]
        L.hevcdbk_synchronize.argtypes = [VP]
        L.hevcdbk_compute_stream.argtypes = [VP]
        L.hevcdbk_compute_stream.restype = VP
        L.hevcdbk_h265_filter_device_g4.argtypes = [VP, C.POINTER(L0.DevicePlanes), C.c_int, C.c_int, C.c_uint, C.POINTER(L0.H265Params), C.c_int,
                                                    C.POINTER(L0.SliceOffsets), VP]
        self.has_sp = hasattr(L, "hevcdbk_h265_filter_device_sp")
        if self.has_sp:
            L.hevcdbk_h265_filter_device_sp.argtypes = [VP, C.POINTER(L0.DevicePlanes), C.c_uint, C.POINTER(L0.H265Params), C.c_int,
                                                        C.POINTER(L0.SliceOffsets), VP]
        h = VP()
        rc = L.hevcdbk_create(0, C.byref(h))
        if rc:
            raise SystemExit("%s: hevcdbk_create -> %d" % (path, rc))
        self.h = h
        self.stream = L.hevcdbk_compute_stream(h)   # where a call without a stream of the caller's enqueues


class Events:
    """two events of the HIP runtime the libraries run on, recorded on a library's stream around a run of calls"""

    def __init__(self):
        hip = self.hip = C.CDLL("libamdhip64.so")
        hip.hipEventRecord.argtypes = [VP, VP]
        hip.hipEventSynchronize.argtypes = [VP]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), VP, VP]
        self.e = [VP(), VP()]
        for e in self.e:
            assert hip.hipEventCreate(C.byref(e)) == 0

    def start(self, stream):
        assert self.hip.hipEventRecord(self.e[0], stream) == 0

    def stop_ms(self, stream):
        assert self.hip.hipEventRecord(self.e[1], stream) == 0
        assert self.hip.hipEventSynchronize(self.e[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.e[0], self.e[1]) == 0
        return float(ms.value)


def planes_of(pool, w, h, n, bd, qp_map):
    """n frames of the w x h chroma planes of a 2w x 2h picture, as two planar planes and as one plane of pairs, with the operands they
    share -> (DevicePlanes planar Cb, planar Cr, pairs; bytes moved per call)"""
    sb = 1 if bd == 8 else 2
    comps = []
    for k in range(2):
        src = np.stack([synth.blocky_plane(w, h, seed=7 + k, frame=f, bit_depth=bd) for f in range(4)])
        comps.append(np.concatenate([src] * (n // 4 + 1))[:n])
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    vb[:, 1:(w - 1) // 8 + 1] = 2
    hb = np.zeros((h // 8 + 1, w // 4), np.uint8)
    hb[1:(h - 1) // 8 + 1, :] = 2
    dv, dh = pool.up(vb), pool.up(hb)
    dm = pool.up(synth.ctu_qp_map(2 * w, 2 * h, seed=29, lo=26, hi=38, ctu_log2=4)) if qp_map else None
    out = []
    for frames, rw in ((comps[0], w), (comps[1], w), (np.stack(comps, axis=-1).reshape(n, h, 2 * w), 2 * w)):
        p = L0.DevicePlanes()
        p.src, p.dst = pool.up(frames), pool.alloc(frames.nbytes)
        p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = rw * sb, rw * h * sb, n, w, h
        p.bit_depth, p.sample_bytes, p.is_chroma = bd, sb, 1
        p.vert_bs, p.hor_bs = dv, dh
        if dm:
            p.qp_map, p.qp_map_stride, p.ctu_log2 = dm, (2 * w + 15) // 16, 4
        out.append(p)
    return out, 4 * comps[0].nbytes


def passes(w, h, n, bd, steps):
    """what a caller of the planar entries pays around them: pairs -> two planes and two planes -> pairs, beside a plain copy of the
    same bytes (tools/ubench/sp_passes, a process of its own, run before this one touches the device); None if it is not built"""
    exe = os.path.join(ROOT, "tools", "ubench", "sp_passes")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe, str(w), str(h), str(n), "1" if bd == 8 else "2", str(steps)], capture_output=True, text=True, timeout=120)
    return json.loads(out.stdout) if out.returncode == 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", help="libhevcdbk.so of the build to compare against (it runs the two planar launches)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gpu_video_codec_amd", "libhevcdbk.so"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--bit-depth", type=int, action="append", default=None)
    ap.add_argument("--size", action="append", default=None, help="WxH of the PICTURE (default 1920x1080 and 3840x2160)")
    ap.add_argument("--passes", action="store_true", help="also time the split / merge passes a caller of the planar entries needs")
    a = ap.parse_args()
    sizes = [tuple(int(x) for x in s.split("x")) for s in (a.size or ["1920x1080", "3840x2160"])]
    depths = a.bit_depth or [8, 10]
    extras = {(W, H, bd): passes(W // 2, H // 2, a.frames, bd, a.steps) for (W, H) in sizes for bd in depths} if a.passes else {}
    old, new = Lib(a.parent), Lib(a.lib)
    if not new.has_sp:
        raise SystemExit("%s has no _sp entry" % a.lib)
    pool = Pool(new)
    ev = Events()
    n = a.frames
    hp = L0.H265Params(0, 0, -2, 3)
    for (W, H) in sizes:
        w, h = W // 2, H // 2
        for bd in depths:
            extra = extras.get((W, H, bd))
            for name, qp_map in (("deblock", False), ("deblock", True)):
                (pcb, pcr, psp), nbytes = planes_of(pool, w, h, n, bd, qp_map)

                def planar(lib):
                    return (lib.L.hevcdbk_h265_filter_device_g4(lib.h, C.byref(pcb), 1, 1, a.qp, C.byref(hp), L0.KERNEL_PACKED, None, None) or
                            lib.L.hevcdbk_h265_filter_device_g4(lib.h, C.byref(pcr), 2, 1, a.qp, C.byref(hp), L0.KERNEL_PACKED, None, None))

                def sp(lib):
                    return lib.L.hevcdbk_h265_filter_device_sp(lib.h, C.byref(psp), a.qp, C.byref(hp), L0.KERNEL_PACKED, None, None)

                variants = [("a_parent_planar", old, planar), ("b_this_planar", new, planar), ("c_this_sp", new, sp),
                            ("a_parent_planar_again", old, planar)]
                ms = {k: [] for k, *_ in variants}
                wall = {k: [] for k, *_ in variants}
                for k, lib, fn in variants:   # settle the clocks, and every variant must be taken
                    for _ in range(150):
                        rc = fn(lib)
                        if rc:
                            raise SystemExit("%s %s -> %d" % (name, k, rc))
                    lib.L.hevcdbk_synchronize(lib.h)
                for r in range(a.rounds):
                    for k, lib, fn in (variants if r % 2 == 0 else variants[::-1]):
                        for _ in range(20):
                            fn(lib)
                        lib.L.hevcdbk_synchronize(lib.h)
                        t0 = time.perf_counter()
                        ev.start(lib.stream)
                        for _ in range(a.steps):
                            fn(lib)
                        ms[k].append(ev.stop_ms(lib.stream) / a.steps)
                        wall[k].append((time.perf_counter() - t0) / a.steps * 1e3)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                spread = abs(med["a_parent_planar"] - med["a_parent_planar_again"])
                yard = max(med["a_parent_planar"], med["a_parent_planar_again"])
                rec = {"workload": "%s: pair plane %dx%d of %dx%d 4:2:0, %d-bit x %d frames, %s" % (
                           name, w, h, W, H, bd, n, "QP map per 16x16" if qp_map else "one QP"),
                       "timing": "events on the stream", "median_ms": {k: round(v, 4) for k, v in med.items()},
                       "wall_ms": {k: round(float(np.median(v)), 4) for k, v in wall.items()}, "spread_ms": round(spread, 4),
                       "sp_minus_parent_ms": round(med["c_this_sp"] - yard, 4), "sp_within_parent_plus_spread": med["c_this_sp"] <= yard + spread,
                       "planar_entry_moved_ms": round(med["b_this_planar"] - yard, 4),
                       "gbytes_per_s_sp": round(nbytes / med["c_this_sp"] / 1e6, 1),
                       "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
                if extra is not None:
                    rec["caller_passes_ms"] = extra
                print(json.dumps(rec), flush=True)
    for lib in (old, new):
        lib.L.hevcdbk_destroy(lib.h)


if __name__ == "__main__":
    main()
