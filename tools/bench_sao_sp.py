#!/usr/bin/env python3
"""Same-process A/B for SAO of a semi-planar chroma plane (hevcdbk_sao_filter_device_sp): what the Cb / Cr pairs of a 4:2:0 picture
cost in ONE launch on the interleaved plane against what a caller had before -- two launches of the planar
hevcdbk_sao_filter_device_g4 on the split planes -- through another build (the parent commit's libhevcdbk.so) and through this one
(whose planar entry must not have moved).

    python3 tools/bench_sao_sp.py parent/libhevcdbk.so [--lib gpu_video_codec_amd/libhevcdbk.so] [--bit-depth 8 --bit-depth 10]

The method is tools/bench_sp.py's: both libraries in ONE process on the same device buffers, taking turns
  a parent_planar   b this_planar   c this_sp   a parent_planar_again
per round (the order reversed every other round), each turn 20 untimed calls and then --steps calls between two events on the library's
own stream, after 150 settling calls of every variant; the wall clock around the same calls beside it.  `spread_ms` = |median(a) -
median(a again)|; the expectation under test is c <= a + spread.  --passes: the split and merge passes a caller of (a) needs
(tools/ubench/sp_passes), which are NOT in (a).
Workloads: the pair planes 960x540 and 1920x1080 (samples per component), --frames frames per call, 32-sample CTBs; parameters
  merged  random types, classes, offsets, merged from the left / upper CTB as a stream's merge flags do (the generator of
          tools/bench_sao.py --merge) -- Cb and Cr of a CTB share type and class, as 7.3.8.3 has it, with their own offsets / band position
  edge    every CTB edge offset (random classes)        band    every CTB band offset
One JSON line per workload, bit depth and parameter set."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_video_codec_amd import _lib as L0, synth  # struct definitions only  # noqa: E402
from bench_g4 import VP, Pool  # noqa: E402
from bench_sp import Events, Lib as SpLib, passes  # noqa: E402

CTB_LOG2 = 5
SAO_G4 = [VP, C.POINTER(L0.DevicePlanes), VP, C.c_uint, C.c_size_t, C.c_uint, C.c_uint, VP, C.c_uint, C.c_size_t, C.POINTER(L0.SaoBorders), VP]
SAO_SP = [VP, C.POINTER(L0.DevicePlanes), VP, VP, C.c_uint, C.c_size_t, C.c_uint, VP, C.c_uint, C.c_size_t, C.POINTER(L0.SaoBorders), VP]


class Lib(SpLib):
    def __init__(self, path):
        super().__init__(path)
        self.L.hevcdbk_sao_filter_device_g4.argtypes = SAO_G4
        self.has_sao_sp = hasattr(self.L, "hevcdbk_sao_filter_device_sp")
        if self.has_sao_sp:
            self.L.hevcdbk_sao_filter_device_sp.argtypes = SAO_SP


def params_of(w, h, kind, bd):
    """(Cb entries, Cr entries) of the w x h grid of 32-sample CTBs"""
    dt = np.dtype(L0.SAO_CTB_DTYPE)
    rng = np.random.RandomState(5)
    rows, cols = (h + 31) // 32, (w + 31) // 32
    both = np.zeros((rows, cols), np.dtype([("cb", dt), ("cr", dt)]))
    typ = rng.randint(0, 3, (rows, cols)) if kind == "merged" else np.full((rows, cols), {"edge": 2, "band": 1}[kind])
    eo = rng.randint(0, 4, (rows, cols))
    for k in ("cb", "cr"):
        both[k]["type"] = typ
        both[k]["cls"] = np.where(typ == 1, rng.randint(0, 32, (rows, cols)), eo)
        both[k]["offset"] = rng.randint(-7, 8, (rows, cols, 4)) << max(bd - 10, 0)
    if kind == "merged":
        from oracle import h265
        both = h265.merge_sao_params(both, seed=18)   # the merge flags are the CTB's: both components take the same neighbour's entries
    return np.ascontiguousarray(both["cb"]), np.ascontiguousarray(both["cr"])


def planes_of(pool, w, h, n, bd):
    """n frames as two planar planes and as one plane of pairs -> (DevicePlanes planar Cb, planar Cr, pairs; bytes moved per call)"""
    sb = 1 if bd == 8 else 2
    comps = []
    for k in range(2):
        src = np.stack([synth.blocky_plane(w, h, seed=7 + k, frame=f, bit_depth=bd) for f in range(4)])
        comps.append(np.concatenate([src] * (n // 4 + 1))[:n])
    out = []
    for frames, rw in ((comps[0], w), (comps[1], w), (np.stack(comps, axis=-1).reshape(n, h, 2 * w), 2 * w)):
        p = L0.DevicePlanes()
        p.src, p.dst = pool.up(frames), pool.alloc(frames.nbytes)
        p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = rw * sb, rw * h * sb, n, w, h
        p.bit_depth, p.sample_bytes, p.is_chroma = bd, sb, 1
        out.append(p)
    return out, 4 * comps[0].nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", help="libhevcdbk.so of the build to compare against (it runs the two planar launches)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gpu_video_codec_amd", "libhevcdbk.so"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bit-depth", type=int, action="append", default=None)
    ap.add_argument("--size", action="append", default=None, help="WxH of the PAIR PLANE, samples per component (default 960x540 and 1920x1080)")
    ap.add_argument("--kind", action="append", default=None, choices=["merged", "edge", "band"])
    ap.add_argument("--passes", action="store_true", help="also time the split / merge passes a caller of the planar entry needs")
    a = ap.parse_args()
    sizes = [tuple(int(x) for x in s.split("x")) for s in (a.size or ["960x540", "1920x1080"])]
    depths = a.bit_depth or [8, 10]
    kinds = a.kind or ["merged", "edge", "band"]
    extras = {(w, h, bd): passes(w, h, a.frames, bd, a.steps) for (w, h) in sizes for bd in depths} if a.passes else {}
    old, new = Lib(a.parent), Lib(a.lib)
    if not new.has_sao_sp:
        raise SystemExit("%s has no _sp SAO entry" % a.lib)
    pool = Pool(new)
    ev = Events()
    n = a.frames
    for (w, h) in sizes:
        cols = (w + 31) // 32
        for bd in depths:
            (pcb, pcr, psp), nbytes = planes_of(pool, w, h, n, bd)
            extra = extras.get((w, h, bd))
            for kind in kinds:
                cb, cr = params_of(w, h, kind, bd)
                dcb, dcr = pool.up(cb), pool.up(cr)

                def planar(lib):
                    return (lib.L.hevcdbk_sao_filter_device_g4(lib.h, C.byref(pcb), dcb, cols, 0, CTB_LOG2, CTB_LOG2, None, 0, 0, None, None) or
                            lib.L.hevcdbk_sao_filter_device_g4(lib.h, C.byref(pcr), dcr, cols, 0, CTB_LOG2, CTB_LOG2, None, 0, 0, None, None))

                def sp(lib):
                    return lib.L.hevcdbk_sao_filter_device_sp(lib.h, C.byref(psp), dcb, dcr, cols, 0, CTB_LOG2, None, 0, 0, None, None)

                variants = [("a_parent_planar", old, planar), ("b_this_planar", new, planar), ("c_this_sp", new, sp),
                            ("a_parent_planar_again", old, planar)]
                ms = {k: [] for k, *_ in variants}
                wall = {k: [] for k, *_ in variants}
                for k, lib, fn in variants:   # settle the clocks, and every variant must be taken
                    for _ in range(150):
                        rc = fn(lib)
                        if rc:
                            raise SystemExit("%s %s -> %d" % (kind, k, rc))
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
                rec = {"workload": "sao: pair plane %dx%d, %d-bit x %d frames, 32-sample CTBs, parameters: %s" % (w, h, bd, n, kind),
                       "timing": "events on the stream", "median_ms": {k: round(v, 4) for k, v in med.items()},
                       "wall_ms": {k: round(float(np.median(v)), 4) for k, v in wall.items()}, "spread_ms": round(spread, 4),
                       "sp_minus_parent_ms": round(med["c_this_sp"] - yard, 4), "sp_within_parent_plus_spread": med["c_this_sp"] <= yard + spread,
                       "planar_entry_moved_ms": round(med["b_this_planar"] - yard, 4),
                       "gbytes_per_s_sp": round(nbytes / med["c_this_sp"] / 1e6, 1),
                       "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}
                if extra is not None:
                    rec["caller_passes_ms"] = extra
                    rec["sp_beats_parent_plus_passes"] = med["c_this_sp"] < yard + extra["split_ms"] + extra["merge_ms"]
                print(json.dumps(rec), flush=True)
    for lib in (old, new):
        lib.L.hevcdbk_destroy(lib.h)


if __name__ == "__main__":
    main()
