#!/usr/bin/env python3
"""Spec-exact mode (H.265 8.7.2) kernel rate on the bench workload (64 x 3840x2160 8-bit luma in HBM, QP 32, bS 2 on every
interior edge), generic vs packed kernel.  Wall clock around back-to-back launches (no per-launch events in this entry);
diagnostic, not bench.py's metric.  Parity of this mode is the business of tests/test_gpu_h265.py."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import deblock, synth, _lib


def slice_offset_operands(ctx, rows, cols, ctb_log2=6):
    """the two operand states of the --slice-offsets legs for a picture of rows x cols CTBs: 'uniform' = one pair everywhere,
    'decoder' = a slice every 8 CTB rows with differing pairs; {name: _lib.SliceOffsets} (the buffers stay allocated)"""
    pairs = [(-2, 1), (3, -3), (0, 2), (-6, 6), (1, 0), (5, -5)]   # (slice_beta_offset_div2, slice_tc_offset_div2)
    uni = np.zeros((rows, cols, 2), np.int8)
    uni[...] = pairs[0]
    dec = np.zeros((rows, cols, 2), np.int8)
    for r in range(rows):
        dec[r, :] = pairs[(r // 8) % len(pairs)]
    out = {}
    for name, arr in (("uniform", uni), ("decoder", dec)):
        d = ctx.alloc(arr.nbytes)
        d.upload(arr.view(np.uint8).ravel())
        out[name] = _lib.SliceOffsets(d.ptr, cols, 0, ctb_log2)
        out[name]._buf = d
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--qp-map", type=int, default=0, metavar="LOG2",
                    help="QP per unit of (1 << LOG2) luma samples, qp-6 .. qp+6 (3..6; 0 = one QP): what a stream with cu_qp_delta has")
    ap.add_argument("--bs", choices=["2", "mixed"], default="2", help="bS 2 on every interior edge, or a seeded mix of 0 / 1 / 2 per 4-sample segment")
    ap.add_argument("--only", choices=["generic", "packed"], default=None)
    ap.add_argument("--chroma-format", choices=["420", "422", "444"], default=None,
                    help="time the Cb plane of a picture of this format (the QP map stays in luma units) instead of the luma plane")
    ap.add_argument("--bit-depth", type=int, default=8, help="8, or 10 / 12 in 16-bit containers")
    ap.add_argument("--slice-offsets", action="store_true",
                    help="per-slice deblocking offsets (hevcdbk_h265_filter_device_sl, CtbSizeY 64): the call without the operand, with one "
                         "pair everywhere, with a slice every 8 CTB rows with differing pairs, and without it again take turns in this one "
                         "process on the same buffers; the median of --rounds rounds each")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--g4", action="store_true",
                    help="the _g4 entry (hevcdbk_h265_filter_device_g4): with --chroma-format it takes chroma planes sized in multiples of 4, "
                         "e.g. --width 1920 --height 1080 --chroma-format 420 for the 960x540 Cb plane")
    a = ap.parse_args()
    n = a.frames
    fmt = a.chroma_format
    sub = {None: (1, 1), "420": (2, 2), "422": (2, 1), "444": (1, 1)}[fmt]
    w, h = a.width // sub[0], a.height // sub[1]  # the timed plane
    ctx = deblock.Context(0)
    b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=a.bit_depth, per_frame_bs=False, is_chroma=fmt is not None)
    kw = {} if fmt is None else {"c_idx": 1, "chroma_format": fmt}
    if a.g4:
        kw["g4"] = True
    distinct = min(n, 8)
    src = np.stack([synth.blocky_plane(w, h, seed=7, frame=i, bit_depth=a.bit_depth) for i in range(distinct)])
    b.upload_all(np.concatenate([src] * (n // distinct + 1))[:n])
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    ex, ey = (w - 1) // 8, (h - 1) // 8   # the last interior edge: x = 8 ex < w (w / 8 - 1 for a multiple of 8, w / 8 for 8k + 4)
    vb[:, 1:ex + 1] = 2
    hb = np.zeros((h // 8 + 1, w // 4), np.uint8)
    hb[1:ey + 1, :] = 2
    if a.bs == "mixed":
        rng = np.random.RandomState(3)
        vb[:, 1:ex + 1] = rng.randint(0, 3, (h // 4, ex))
        hb[1:ey + 1, :] = rng.randint(0, 3, (ey, w // 4))
    dv, dh = ctx.alloc(vb.size), ctx.alloc(hb.size)
    dv.upload(vb)
    dh.upload(hb)
    p = b.planes()
    p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
    bytes_per_launch = n * (2 * w * h * b.sb + vb.size + hb.size)
    if a.qp_map:
        qmap = synth.ctu_qp_map(a.width, a.height, seed=29, lo=max(a.qp - 6, 0), hi=min(a.qp + 6, 51), ctu_log2=a.qp_map)
        dm = ctx.alloc(qmap.nbytes)
        dm.upload(qmap)
        p.qp_map, p.qp_map_stride, p.ctu_log2, p.qp_map_frame_stride = dm.ptr, qmap.shape[1], a.qp_map, 0
        bytes_per_launch += n * qmap.size
    for name, variant in (("generic", _lib.KERNEL_GENERIC), ("packed", _lib.KERNEL_PACKED)):
        if a.only and a.only != name:
            continue
        if a.slice_offsets:
            ops = slice_offset_operands(ctx, (a.height + 63) // 64, (a.width + 63) // 64)
            variants = [("none", None), ("uniform", ops["uniform"]), ("decoder", ops["decoder"]), ("none_again", None)]
            ms = {k: [] for k, _ in variants}
            for _ in range(300):  # settle the clocks
                ctx.filter_device_h265(p, a.qp, variant=variant, **kw)
            ctx.synchronize()
            for _ in range(a.rounds):
                for k, so in variants:
                    for _ in range(20):
                        ctx.filter_device_h265(p, a.qp, variant=variant, slice_offsets=so, **kw)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        ctx.filter_device_h265(p, a.qp, variant=variant, slice_offsets=so, **kw)
                    ctx.synchronize()
                    ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            print(json.dumps({"mode": "h265", "kernel": name, "slice_offsets": True, "ms": med, "rounds_ms": ms,
                              "spread_ms": abs(med["none"] - med["none_again"]),
                              "ratio_to_none": {k: med[k] / med["none"] for k in ("uniform", "decoder", "none_again")},
                              "workload": "%dx%d %d-bit %s x %d, QP %d%s, bS %s" % (w, h, a.bit_depth, "luma" if fmt is None else "Cb of %s" % fmt, n, a.qp, " +-6 per %d x %d unit" % (1 << a.qp_map, 1 << a.qp_map) if a.qp_map else "", a.bs)}))
            continue
        for _ in range(100):
            ctx.filter_device_h265(p, a.qp, variant=variant, **kw)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ctx.filter_device_h265(p, a.qp, variant=variant, **kw)
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        print(json.dumps({"mode": "h265", "kernel": name, "ms_per_launch": dt * 1e3, "frames_per_s": n / dt,
                          "GBps": bytes_per_launch / dt * 1e-9, "frac_of_8TBps": bytes_per_launch / dt / 8e12,
                          "workload": "%dx%d %d-bit %s x %d, QP %d%s, bS %s" % (w, h, a.bit_depth, "luma" if fmt is None else "Cb of %s" % fmt, n, a.qp, " +-6 per %d x %d unit" % (1 << a.qp_map, 1 << a.qp_map) if a.qp_map else "", a.bs)}))


if __name__ == "__main__":
    main()
