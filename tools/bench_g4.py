#!/usr/bin/env python3
"""Same-process A/B for planes sized in multiples of 4 (the _g4 entries): what a 1920x1080 4:2:0 picture costs through the _g4 entries
of THIS build against the workaround a caller needed before -- the picture padded to 1920x1088 (chroma 960x544) through the entries of
another build (the parent commit's libhevcdbk.so) -- and, beside them, the multiple-of-8 call through the existing entries of this
build (which must not have moved).

    python3 tools/bench_g4.py parent/libhevcdbk.so [--lib gpu_video_codec_amd/libhevcdbk.so] [--bit-depth 8 --bit-depth 10]

Both libraries are loaded into ONE process (ctypes, RTLD_LOCAL), work on the same device buffers and take turns
  parent  this_mult8  this_g4  parent_again
per round: each turn 20 untimed calls, then --steps back-to-back calls and one synchronisation, wall clock.  Reported per workload: the
median over --rounds of every variant, and `spread_ms` = |median(parent) - median(parent_again)|, the run-to-run spread of the yardstick.
Workloads, --frames frames per call, bS 2 on every interior edge, one QP and a QP map per 16x16 luma samples:
  picture  Y + Cb + Cr, deblocking + SAO in one launch (seeded per-CTB parameters, CtbSizeY 64)
  chroma   the packed deblocking kernel on the Cb plane (src -> dst)
  sao      the SAO pass on the Cb plane
One JSON line per workload and bit depth."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_video_codec_amd import _lib as L0, synth  # struct definitions only  # noqa: E402

VP = C.c_void_p


class Lib:
    def __init__(self, path):
        self.path = os.path.abspath(path)
        L = self.L = C.CDLL(self.path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
        L.hevcdbk_create.argtypes = [C.c_int, C.POINTER(VP)]
        L.hevcdbk_destroy.argtypes = [VP]
        L.hevcdbk_device_malloc.argtypes = [VP, C.c_size_t, C.POINTER(VP)]
        L.hevcdbk_memcpy_h2d.argtypes = [VP, VP, VP, C.c_size_t]
        L.hevcdbk_synchronize.argtypes = [VP]
        planes = [VP, C.POINTER(L0.DevicePlanes), C.c_uint, C.c_int, C.c_uint, C.POINTER(L0.H265Params), C.POINTER(L0.SaoPlaneCf), C.c_int,
                  C.POINTER(L0.SaoBorders), C.POINTER(L0.SliceOffsets), VP]
        filt = [VP, C.POINTER(L0.DevicePlanes), C.c_int, C.c_int, C.c_uint, C.POINTER(L0.H265Params), C.c_int, C.POINTER(L0.SliceOffsets), VP]
        sao = [VP, C.POINTER(L0.DevicePlanes), VP, C.c_uint, C.c_size_t, C.c_uint, C.c_uint, VP, C.c_uint, C.c_size_t,
               C.POINTER(L0.SaoBorders), VP]
        L.hevcdbk_h265_deblock_sao_device_planes_sl.argtypes = planes
        L.hevcdbk_h265_filter_device_sl.argtypes = filt
        L.hevcdbk_sao_filter_device_nox.argtypes = sao
        self.has_g4 = hasattr(L, "hevcdbk_h265_filter_device_g4")
        if self.has_g4:
            L.hevcdbk_h265_deblock_sao_device_planes_g4.argtypes = planes
            L.hevcdbk_h265_filter_device_g4.argtypes = filt
            L.hevcdbk_sao_filter_device_g4.argtypes = sao
        h = VP()
        rc = L.hevcdbk_create(0, C.byref(h))
        if rc:
            raise SystemExit("%s: hevcdbk_create -> %d" % (path, rc))
        self.h = h


class Pool:
    """device memory, allocated through one library's context and used by both"""

    def __init__(self, lib):
        self.lib = lib

    def alloc(self, n):
        p = VP()
        assert self.lib.L.hevcdbk_device_malloc(self.lib.h, max(n, 1), C.byref(p)) == 0
        return p.value

    def up(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        assert self.lib.L.hevcdbk_memcpy_h2d(self.lib.h, d, a.ctypes.data, a.nbytes) == 0
        return d


def picture(pool, W, H, n, bd, qp_map, seed=5):
    """the planes of n frames of a W x H 4:2:0 picture with their operands -> (DevicePlanes[3], SaoPlaneCf[3], bytes moved per call)"""
    sb = 1 if bd == 8 else 2
    planes = (L0.DevicePlanes * 3)()
    sao = (L0.SaoPlaneCf * 3)()
    rng = np.random.RandomState(seed)
    dm = pool.up(synth.ctu_qp_map(W, H, seed=29, lo=26, hi=38, ctu_log2=4)) if qp_map else None
    nbytes = 0
    for i in range(3):
        w, h = (W, H) if i == 0 else (W // 2, H // 2)
        src = np.stack([synth.blocky_plane(w, h, seed=7 + i, frame=k, bit_depth=bd) for k in range(4)])
        frames = np.concatenate([src] * (n // 4 + 1))[:n]
        p = planes[i]
        p.src, p.dst = pool.up(frames), pool.alloc(frames.nbytes)
        p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = w * sb, w * h * sb, n, w, h
        p.bit_depth, p.sample_bytes, p.is_chroma = bd, sb, int(i > 0)
        vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
        vb[:, 1:(w - 1) // 8 + 1] = 2
        hb = np.zeros((h // 8 + 1, w // 4), np.uint8)
        hb[1:(h - 1) // 8 + 1, :] = 2
        p.vert_bs, p.hor_bs = pool.up(vb), pool.up(hb)
        if dm:
            p.qp_map, p.qp_map_stride, p.ctu_log2 = dm, (W + 15) // 16, 4
        lg = 6 if i == 0 else 5
        rows, cols = -(-h >> lg), -(-w >> lg)
        prm = np.zeros((rows, cols), np.dtype(L0.SAO_CTB_DTYPE))
        prm["type"] = rng.randint(0, 3, (rows, cols))
        prm["cls"] = np.where(prm["type"] == 1, rng.randint(0, 32, (rows, cols)), rng.randint(0, 4, (rows, cols)))
        prm["offset"] = rng.randint(-7, 8, (rows, cols, 4))
        sao[i].params, sao[i].params_stride, sao[i].ctb_log2_w, sao[i].ctb_log2_h = pool.up(prm), cols, lg, lg
        nbytes += 2 * frames.nbytes
    return planes, sao, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", help="libhevcdbk.so of the build to compare against (it runs the padded picture)")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gpu_video_codec_amd", "libhevcdbk.so"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080, help="the picture; the yardstick is this height rounded up to a multiple of 16")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--bit-depth", type=int, action="append", default=None)
    ap.add_argument("--only", choices=["picture", "chroma", "sao"], action="append", default=None)
    a = ap.parse_args()
    old, new = Lib(a.parent), Lib(a.lib)
    if not new.has_g4:
        raise SystemExit("%s has no _g4 entries" % a.lib)
    pool = Pool(new)
    W, H, HP, n = a.width, a.height, (a.height + 15) // 16 * 16, a.frames
    hp = L0.H265Params(0, 0, 0, 0)
    for bd in a.bit_depth or [8, 10]:
        for qp_map in (False, True):
            pad, sao_pad, bytes_pad = picture(pool, W, HP, n, bd, qp_map)
            g4, sao_g4, bytes_g4 = picture(pool, W, H, n, bd, qp_map)
            work = {
                "picture": lambda lib, pl, so, e: getattr(lib.L, "hevcdbk_h265_deblock_sao_device_planes_" + e)(
                    lib.h, pl, 3, 1, a.qp, C.byref(hp), so, L0.FUSED_ON, None, None, None),
                "chroma": lambda lib, pl, so, e: getattr(lib.L, "hevcdbk_h265_filter_device_" + e)(
                    lib.h, C.byref(pl[1]), 1, 1, a.qp, C.byref(hp), L0.KERNEL_PACKED, None, None),
                "sao": lambda lib, pl, so, e: getattr(lib.L, "hevcdbk_sao_filter_device_" + ("g4" if e == "g4" else "nox"))(
                    lib.h, C.byref(pl[1]), so[1].params, so[1].params_stride, 0, 5, 5, None, 0, 0, None, None),
            }
            for name, fn in work.items():
                if a.only and name not in a.only:
                    continue
                variants = [("parent_padded", old, pad, sao_pad, "sl"), ("this_padded", new, pad, sao_pad, "sl"),
                            ("this_g4", new, g4, sao_g4, "g4"), ("parent_padded_again", old, pad, sao_pad, "sl")]
                ms = {k: [] for k, *_ in variants}
                for k, lib, pl, so, e in variants:   # settle the clocks, and every variant must be taken
                    for _ in range(150):
                        rc = fn(lib, pl, so, e)
                        if rc:
                            raise SystemExit("%s %s -> %d" % (name, k, rc))
                    lib.L.hevcdbk_synchronize(lib.h)
                for r in range(a.rounds):
                    for k, lib, pl, so, e in (variants if r % 2 == 0 else variants[::-1]):
                        for _ in range(20):
                            fn(lib, pl, so, e)
                        lib.L.hevcdbk_synchronize(lib.h)
                        t0 = time.perf_counter()
                        for _ in range(a.steps):
                            fn(lib, pl, so, e)
                        lib.L.hevcdbk_synchronize(lib.h)
                        ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
                med = {k: float(np.median(v)) for k, v in ms.items()}
                spread = abs(med["parent_padded"] - med["parent_padded_again"])
                yard = max(med["parent_padded"], med["parent_padded_again"])
                print(json.dumps({"workload": "%s: %dx%d 4:2:0 %d-bit x %d frames, %s, bS 2 everywhere; padded = %dx%d" % (
                                      name, W, H, bd, n, "QP map per 16x16" if qp_map else "one QP", W, HP),
                                  "median_ms": {k: round(v, 4) for k, v in med.items()}, "spread_ms": round(spread, 4),
                                  "g4_minus_parent_ms": round(med["this_g4"] - yard, 4), "g4_within_parent_plus_spread": med["this_g4"] <= yard + spread,
                                  "existing_entry_moved_ms": round(med["this_padded"] - yard, 4),
                                  "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                  "bytes_g4_over_padded": round(bytes_g4 / bytes_pad, 4)}), flush=True)
    for lib in (old, new):
        lib.L.hevcdbk_destroy(lib.h)


if __name__ == "__main__":
    main()
