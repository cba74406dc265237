#!/usr/bin/env python3
"""Deblocking + SAO of F x 3840x2160 8-bit luma planes in HBM, src -> dst, in one call: the fused kernel
(hevc_deblock_sao_device, one workgroup = one 192x128 tile through LDS) against the two launches it replaces
(HEVCDBK_FUSED_OFF: deblocking into the context's scratch plane, then the SAO pass).  Seeded per-CTB SAO parameters (one
third off / band / edge, or --types), wall clock over back-to-back calls after a settling period.  Diagnostic."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import deblock, synth, _lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--mode", choices=["ref", "h265"], default="ref")
    ap.add_argument("--types", default="mix")
    ap.add_argument("--diag", action="append", default=None,
                    help="diagnostic library with these knobs (csrc/hevcdbk_diag.h), e.g. noswz; may be given several times: one result per knob set")
    ap.add_argument("--chroma-format", choices=["420", "422", "444"], default=None,
                    help="--mode h265: Y + Cb + Cr of pictures of this format in one call (CtbSizeY 64) instead of luma planes")
    ap.add_argument("--bit-depth", type=int, default=8, help="luma planes: 8, or 10 / 12 in 16-bit containers")
    ap.add_argument("--borders", choices=["none", "zero", "decoder", "every-ctb"], default=None,
                    help="--mode h265: slice / tile boundaries SAO must not look across (the _nox entries; tools/sao_border_layouts.py): the fused "
                         "call without the operand, with this layout and without it again take turns in this one process on the same buffers")
    ap.add_argument("--slice-offsets", action="store_true",
                    help="--mode h265: per-slice deblocking offsets (the _sl entries, CtbSizeY 64): the fused call without the operand, with one pair "
                         "everywhere, with a slice every 8 CTB rows with differing pairs, and without it again take turns in this one process; "
                         "with --borders every one of the four carries that layout (the _nox kernels are then the yardstick)")
    ap.add_argument("--rounds", type=int, default=3, help="--borders / --slice-offsets: rounds of turns; the median of each variant is reported")
    ap.add_argument("--g4", action="store_true",
                    help="--mode h265 --chroma-format F: the _g4 entry (hevcdbk_h265_deblock_sao_device_planes_g4), which takes chroma planes "
                         "sized in multiples of 4: --width 1920 --height 1080 --chroma-format 420 is Y 1920x1080 with Cb, Cr 960x540")
    a = ap.parse_args()
    if a.g4 and not a.chroma_format:
        ap.error("--g4 needs --mode h265 --chroma-format (a luma plane is a multiple of 8)")
    if a.borders is not None and a.mode != "h265":
        ap.error("--borders needs --mode h265 (the reference-exact mode has no slices or tiles)")
    if a.slice_offsets and a.mode != "h265":
        ap.error("--slice-offsets needs --mode h265")
    if a.chroma_format and a.mode != "h265":
        ap.error("--chroma-format needs --mode h265 (the reference-exact mode is 4:2:0 only)")
    if a.diag is not None:
        _lib.use_diagnostic_library(a.diag[0] or None)
    w, h, n = a.width, a.height, a.frames
    ctx = deblock.Context(0)
    b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=a.bit_depth, per_frame_bs=False)
    src = np.stack([synth.blocky_plane(w, h, seed=7, frame=i, bit_depth=a.bit_depth) for i in range(4)])
    b.upload_all(np.concatenate([src] * (n // 4 + 1))[:n])
    rng = np.random.RandomState(5)
    rows, cols = (h + 63) // 64, (w + 63) // 64
    prm = np.zeros((rows, cols), np.dtype(_lib.SAO_CTB_DTYPE))
    prm["type"] = rng.randint(0, 3, (rows, cols))
    if a.types != "mix":
        prm["type"] = {"off": 0, "band": 1, "edge": 2}[a.types]
    prm["cls"] = np.where(prm["type"] == 1, rng.randint(0, 32, (rows, cols)), rng.randint(0, 4, (rows, cols)))
    prm["offset"] = rng.randint(-7, 8, (rows, cols, 4))
    dp = ctx.alloc(prm.nbytes)
    dp.upload(prm.view(np.uint8).ravel())
    p = b.planes()
    if a.mode == "h265":
        L = _lib.lib()
        nv, nh = L.hevcdbk_h265_num_vert_bs(w, h), L.hevcdbk_h265_num_hor_bs(w, h)
        dv, dh = ctx.alloc(nv), ctx.alloc(nh)
        dv.upload(np.full(nv, 2, np.uint8))
        dh.upload(np.full(nh, 2, np.uint8))
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0

    nbytes = 2 * n * w * h * b.sb
    if a.chroma_format:  # the planes of tools/bench_rext.py: bS 2 everywhere, seeded SAO parameters per plane
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import bench_rext
        yuv, sao, nbytes, _keep = bench_rext.setup(ctx, a.chroma_format, w, h, n, a.bit_depth, np.random.RandomState(5))
        h265 = {"tc_offset_div2": 0, "beta_offset_div2": 0, "cb_qp_offset": 0, "cr_qp_offset": 0}

    def call(fused, borders=None, slice_offsets=None):
        if a.chroma_format:
            ctx.deblock_sao_device_planes(yuv, a.qp, sao, h265=h265, fused=fused, chroma_format=a.chroma_format, borders=borders,
                                          slice_offsets=slice_offsets, g4=a.g4)
        elif a.mode == "ref":
            ctx.deblock_sao_device(p, a.qp, dp.ptr, cols, 6, fused=fused)
        else:
            ctx.deblock_sao_h265_device(p, a.qp, dp.ptr, cols, 6, fused=fused, borders=borders, slice_offsets=slice_offsets)

    what = "luma" if not a.chroma_format else "Y+Cb+Cr %s" % a.chroma_format
    if a.borders is not None and not a.slice_offsets:  # none / the layout / none again, taking turns; `spread` = the distance between the two runs without the operand
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import sao_border_layouts as sbl
        bo, _buf, share = sbl.device_borders(ctx, a.borders, rows, cols)
        variants = [("none", None), (a.borders, bo), ("none_again", None)]
        ms = {k: [] for k, _ in variants}
        for _ in range(300):  # settle the clocks
            call(_lib.FUSED_ON)
        ctx.synchronize()
        for _ in range(a.rounds):
            for k, bb in variants:
                for _ in range(20):
                    call(_lib.FUSED_ON, bb)
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(_lib.FUSED_ON, bb)
                ctx.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({"stage": "deblock+sao", "mode": a.mode, "borders": a.borders, "masked_region_share": share, "ms": med, "rounds_ms": ms,
                          "spread_ms": abs(med["none"] - med["none_again"]),
                          "frac_of_8TBps_read_once_write_once": {k: nbytes / (v * 1e-3) / 8e12 for k, v in med.items()},
                          "workload": "%dx%d %d-bit %s x %d, QP %d, CTB types: %s" % (w, h, a.bit_depth, what, n, a.qp, a.types)}))
        return

    if a.slice_offsets:  # none / uniform / decoder / none again, taking turns (as --borders)
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import bench_h265
        ops = bench_h265.slice_offset_operands(ctx, rows, cols)
        bo = None
        if a.borders is not None:
            import sao_border_layouts as sbl
            bo, _buf, _share = sbl.device_borders(ctx, a.borders, rows, cols)
        variants = [("none", None), ("uniform", ops["uniform"]), ("decoder", ops["decoder"]), ("none_again", None)]
        ms = {k: [] for k, _ in variants}
        for _ in range(300):  # settle the clocks
            call(_lib.FUSED_ON)
        ctx.synchronize()
        for _ in range(a.rounds):
            for k, so in variants:
                for _ in range(20):
                    call(_lib.FUSED_ON, bo, so)
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(_lib.FUSED_ON, bo, so)
                ctx.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(json.dumps({"stage": "deblock+sao", "mode": a.mode, "slice_offsets": True, "borders": a.borders, "ms": med, "rounds_ms": ms,
                          "spread_ms": abs(med["none"] - med["none_again"]),
                          "ratio_to_none": {k: med[k] / med["none"] for k in ("uniform", "decoder", "none_again")},
                          "workload": "%dx%d %d-bit %s x %d, QP %d, CTB types: %s" % (w, h, a.bit_depth, what, n, a.qp, a.types)}))
        return

    out = {}
    runs = [("fused", _lib.FUSED_ON, None), ("two_launches", _lib.FUSED_OFF, None), ("fused_again", _lib.FUSED_ON, None)]
    if a.diag is not None:
        runs = [("fused[%s]" % k, _lib.FUSED_ON, k) for k in a.diag] * 2
    for name, fused, knobs in runs:
        if knobs is not None:
            _lib.use_diagnostic_library(knobs or None)
            if name in out:
                name += " again"
        for _ in range(max(a.steps, 100)):
            call(fused)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            call(fused)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        out[name] = {"ms_per_step": dt * 1e3, "frames_per_s": n / dt, "frac_of_8TBps_read_once_write_once": nbytes / dt / 8e12}
    print(json.dumps({"stage": "deblock+sao", "mode": a.mode, "workload": "%dx%d 8-bit %s x %d, QP %d, CTB types: %s" % (w, h, what, n, a.qp, a.types),
                      **out}))


if __name__ == "__main__":
    main()
