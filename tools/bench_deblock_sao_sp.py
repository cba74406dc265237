#!/usr/bin/env python3
"""Same-process A/B for deblocking + SAO of a semi-planar picture in one kernel: what the plane of Cb / Cr pairs costs through
hevcdbk_h265_deblock_sao_device_sp_fused, and a whole frame through hevcdbk_h265_deblock_sao_device_nv12, against what a caller had
before -- hevcdbk_h265_deblock_sao_device_sp (two launches) and, for a frame, hevcdbk_h265_deblock_sao_device_planes_g4 on Y alone plus
that chain -- through another build (the parent commit's libhevcdbk.so) and through this one (whose old entries must not have moved).

    python3 tools/bench_deblock_sao_sp.py parent/libhevcdbk.so [--lib gpu_video_codec_amd/libhevcdbk.so] [--bit-depth 8 --bit-depth 10]

The method is tools/bench_sao_sp.py's: both libraries in ONE process on the same device buffers, taking turns
  a parent_two_launches   b this_two_launches   c this_fused   a parent_two_launches_again
per round (the order reversed every other round), each turn 20 untimed calls and then --steps calls between two events on the library's
own stream, after 150 settling calls of every variant.  `spread_ms` = |median(a) - median(a again)|; the expectation under test is
c <= a + spread, with b within spread of a.  Workloads: the pair planes 960x540 and 1920x1080 (samples per component) alone, and the
frames Y 1920x1088 / 3840x2160 with their pair planes; --frames frames per call; 8 and 10 bit; one QP and a map per 16x16; every edge
bS 2; 32-sample chroma CTBs (64-sample luma CTBs) with parameters merged from the left / upper CTB as a stream's merge flags do.
One JSON line per workload."""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_video_codec_amd import _lib as L0, synth  # struct definitions only  # noqa: E402
from bench_g4 import VP, Pool  # noqa: E402
from bench_sp import Events, Lib as SpLib  # noqa: E402

P_PLANES, P_H265, P_BORDERS, P_SLICES = C.POINTER(L0.DevicePlanes), C.POINTER(L0.H265Params), C.POINTER(L0.SaoBorders), C.POINTER(L0.SliceOffsets)
CHAIN_SP = [VP, P_PLANES, C.c_uint, P_H265, VP, VP, C.c_uint, C.c_size_t, C.c_uint, VP, C.c_uint, C.c_size_t, C.c_int, P_BORDERS, P_SLICES, VP]
PLANES_G4 = [VP, P_PLANES, C.c_uint, C.c_int, C.c_uint, P_H265, C.POINTER(L0.SaoPlaneCf), C.c_int, P_BORDERS, P_SLICES, VP]
NV12 = [VP, P_PLANES, P_PLANES, C.c_uint, P_H265, C.POINTER(L0.SaoPlaneCf), C.POINTER(L0.SaoPlaneSp), C.c_int, P_BORDERS, P_SLICES, VP]


class Lib(SpLib):
    def __init__(self, path):
        super().__init__(path)
        self.L.hevcdbk_h265_deblock_sao_device_sp.argtypes = CHAIN_SP
        self.L.hevcdbk_h265_deblock_sao_device_planes_g4.argtypes = PLANES_G4
        self.has_fused = hasattr(self.L, "hevcdbk_h265_deblock_sao_device_sp_fused")
        if self.has_fused:
            self.L.hevcdbk_h265_deblock_sao_device_sp_fused.argtypes = CHAIN_SP
            self.L.hevcdbk_h265_deblock_sao_device_nv12.argtypes = NV12


def merged_params(w, h, log2, bd, seed, n=1):
    """n arrays of entries of the w x h grid of (1 << log2)-sample CTBs sharing type and class (7.3.8.3), merged as a stream merges them"""
    from oracle import h265
    dt = np.dtype(L0.SAO_CTB_DTYPE)
    rng = np.random.RandomState(seed)
    rows, cols = -(-h >> log2), -(-w >> log2)
    names = ["c%d" % i for i in range(n)]
    both = np.zeros((rows, cols), np.dtype([(k, dt) for k in names]))
    typ, eo = rng.randint(0, 3, (rows, cols)), rng.randint(0, 4, (rows, cols))
    for k in names:
        both[k]["type"] = typ
        both[k]["cls"] = np.where(typ == 1, rng.randint(0, 32, (rows, cols)), eo)
        both[k]["offset"] = rng.randint(-7, 8, (rows, cols, 4)) << max(bd - 10, 0)
    both = h265.merge_sao_params(both, seed=18)
    return [np.ascontiguousarray(both[k]) for k in names]


def plane_of(pool, w, h, n, bd, pairs, seed):
    """n frames of a plane of w x h samples (per component: pairs) with every edge bS 2 -> (DevicePlanes, bytes moved per call)"""
    sb = 1 if bd == 8 else 2
    comps = []
    for k in range(2 if pairs else 1):
        src = np.stack([synth.blocky_plane(w, h, seed=seed + k, frame=f, bit_depth=bd) for f in range(4)])
        comps.append(np.concatenate([src] * (n // 4 + 1))[:n])
    frames, rw = (np.stack(comps, axis=-1).reshape(n, h, 2 * w), 2 * w) if pairs else (comps[0], w)
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    vb[:, 1:(w - 1) // 8 + 1] = 2
    hb = np.zeros((h // 8 + 1, w // 4), np.uint8)
    hb[1:(h - 1) // 8 + 1, :] = 2
    p = L0.DevicePlanes()
    p.src, p.dst = pool.up(frames), pool.alloc(frames.nbytes)
    p.pitch, p.frame_stride, p.n_frames, p.plane_w, p.plane_h = rw * sb, rw * h * sb, n, w, h
    p.bit_depth, p.sample_bytes, p.is_chroma = bd, sb, int(pairs)
    p.vert_bs, p.hor_bs = pool.up(vb), pool.up(hb)
    return p, 2 * frames.nbytes


def with_map(pool, p, W, H, qp_map):
    """a copy of plane p of a W x H picture (luma samples), with a QP map per 16x16 or none"""
    q = L0.DevicePlanes.from_buffer_copy(p)
    if qp_map:
        q.qp_map, q.qp_map_stride, q.ctu_log2 = pool.up(synth.ctu_qp_map(W, H, seed=29, lo=26, hi=38, ctu_log2=4)), (W + 15) // 16, 4
    return q


def measure(variants, a, ev, what, nbytes):
    """variants: [(name, lib, fn)] with the yardstick first and again last, the variant under test third"""
    ms = {k: [] for k, *_ in variants}
    for k, lib, fn in variants:   # settle the clocks, and every variant must be taken
        for _ in range(150):
            rc = fn(lib)
            if rc:
                raise SystemExit("%s %s -> %d" % (what, k, rc))
        lib.L.hevcdbk_synchronize(lib.h)
    for r in range(a.rounds):
        for k, lib, fn in (variants if r % 2 == 0 else variants[::-1]):
            for _ in range(20):
                fn(lib)
            lib.L.hevcdbk_synchronize(lib.h)
            ev.start(lib.stream)
            for _ in range(a.steps):
                fn(lib)
            ms[k].append(ev.stop_ms(lib.stream) / a.steps)
    (ka, _, _), (kb, _, _), (kc, _, _), (ka2, _, _) = variants
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = abs(med[ka] - med[ka2])
    yard = max(med[ka], med[ka2])
    print(json.dumps({"workload": what, "timing": "events on the stream", "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "spread_ms": round(spread, 4), "fused_minus_parent_ms": round(med[kc] - yard, 4),
                      "fused_within_parent_plus_spread": med[kc] <= yard + spread, "ratio_parent_over_fused": round(yard / med[kc], 3),
                      "old_entry_moved_ms": round(med[kb] - yard, 4), "old_entry_within_spread": abs(med[kb] - yard) <= spread or med[kb] <= yard,
                      "gbytes_per_s_fused": round(nbytes / med[kc] / 1e6, 1), "rounds_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", help="libhevcdbk.so of the build to compare against")
    ap.add_argument("--lib", default=os.path.join(ROOT, "gpu_video_codec_amd", "libhevcdbk.so"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--bit-depth", type=int, action="append", default=None)
    ap.add_argument("--size", action="append", default=None, help="WxH of the PAIR PLANE, samples per component (default 960x540 and 1920x1080)")
    ap.add_argument("--frame-size", action="append", default=None, help="WxH of Y of a whole frame (default 1920x1088 and 3840x2160)")
    a = ap.parse_args()
    sizes = [tuple(int(x) for x in s.split("x")) for s in (a.size or ["960x540", "1920x1080"])]
    fsizes = [tuple(int(x) for x in s.split("x")) for s in (a.frame_size or ["1920x1088", "3840x2160"])]
    depths = a.bit_depth or [8, 10]
    old, new = Lib(a.parent), Lib(a.lib)
    if not new.has_fused:
        raise SystemExit("%s has no fused _sp entries" % a.lib)
    pool, ev, n = Pool(new), Events(), a.frames
    hp = L0.H265Params(0, 0, 1, -1)
    AUTO, OFF, ON = L0.FUSED_AUTO, L0.FUSED_OFF, L0.FUSED_ON

    def pair_operands(w, h, bd):
        cb, cr = merged_params(w, h, 5, bd, 5, 2)
        return pool.up(cb), pool.up(cr), cb.shape[1]

    def chain(entry, p, dcb, dcr, cols, fused):
        return lambda lib: getattr(lib.L, entry)(lib.h, C.byref(p), a.qp, C.byref(hp), dcb, dcr, cols, 0, 5, None, 0, 0, fused, None, None, None)

    for (w, h) in sizes:
        for bd in depths:
            p0, nbytes = plane_of(pool, w, h, n, bd, True, 7)
            dcb, dcr, cols = pair_operands(w, h, bd)
            for qm in (False, True):
                p = with_map(pool, p0, 2 * w, 2 * h, qm)
                two = chain("hevcdbk_h265_deblock_sao_device_sp", p, dcb, dcr, cols, AUTO)
                fused = chain("hevcdbk_h265_deblock_sao_device_sp_fused", p, dcb, dcr, cols, ON)
                measure([("a_parent_two_launches", old, two), ("b_this_two_launches", new, two), ("c_this_fused", new, fused),
                         ("a_parent_two_launches_again", old, two)], a, ev,
                        "pair plane %dx%d, %d-bit x %d frames, %s" % (w, h, bd, n, "QP map per 16x16" if qm else "one QP"), nbytes)
    for (W, H) in fsizes:
        for bd in depths:
            y0, ybytes = plane_of(pool, W, H, n, bd, False, 3)
            p0, cbytes = plane_of(pool, W // 2, H // 2, n, bd, True, 7)
            dcb, dcr, cols = pair_operands(W // 2, H // 2, bd)
            (yp,) = merged_params(W, H, 6, bd, 9)
            sl = L0.SaoPlaneCf(pool.up(yp), yp.shape[1], 0, 6, 6, None, 0, 0)
            sp = L0.SaoPlaneSp(dcb, dcr, cols, 0, 5, None, 0, 0)
            for qm in (False, True):
                y, p = with_map(pool, y0, W, H, qm), with_map(pool, p0, W, H, qm)
                pairs_two = chain("hevcdbk_h265_deblock_sao_device_sp", p, dcb, dcr, cols, AUTO)

                def per_plane(lib):
                    return (lib.L.hevcdbk_h265_deblock_sao_device_planes_g4(lib.h, C.byref(y), 1, 1, a.qp, C.byref(hp), C.byref(sl), AUTO, None, None, None) or
                            pairs_two(lib))

                def one_launch(lib):
                    return lib.L.hevcdbk_h265_deblock_sao_device_nv12(lib.h, C.byref(y), C.byref(p), a.qp, C.byref(hp), C.byref(sl), C.byref(sp), ON,
                                                                      None, None, None)

                measure([("a_parent_per_plane", old, per_plane), ("b_this_per_plane", new, per_plane), ("c_this_nv12", new, one_launch),
                         ("a_parent_per_plane_again", old, per_plane)], a, ev,
                        "frame Y %dx%d + pairs %dx%d, %d-bit x %d frames, %s" % (W, H, W // 2, H // 2, bd, n, "QP map per 16x16" if qm else "one QP"),
                        ybytes + cbytes)
    for lib in (old, new):
        lib.L.hevcdbk_destroy(lib.h)


if __name__ == "__main__":
    main()
