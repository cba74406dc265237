#!/usr/bin/env python3
"""SAO statistics pass (hevcdbk_sao_stats_device) rate: 64 x 3840x2160 luma in HBM at 8 and 10 bit, on noise, on a blocky picture
and on a flat one (every sample in ONE band bin and in no edge bin: what contention on a bin costs).  The statistics launch and the
existing SAO pass (the leg of tools/bench_sao.py: seeded per-CTB parameters, one third off / band / edge) take turns in this one
process on the same planes; both move two planes' worth of bytes -- the statistics pass reads two, SAO reads one and writes one.
Wall clock over back-to-back launches that end in a synchronise; the median over the rounds is reported, and the spread between
them.  The pick launch is timed once per depth, for the record.  One JSON line per (depth, content).  Diagnostic."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import deblock, synth, _lib


def timed(ctx, fn, steps, warm):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def frames_of(content, w, h, bd, rng):
    """four distinct frames (rec, org)"""
    dt = np.uint8 if bd == 8 else np.uint16
    org = rng.integers(0, 1 << bd, (4, h, w)).astype(dt)
    if content == "noise":
        rec = rng.integers(0, 1 << bd, (4, h, w)).astype(dt)
    elif content == "blocky":
        rec = np.stack([synth.blocky_plane(w, h, seed=7, frame=i, bit_depth=bd) for i in range(4)]).astype(dt)
        org = np.stack([synth.blocky_plane(w, h, seed=8, frame=i, bit_depth=bd) for i in range(4)]).astype(dt)
    else:
        rec = np.full((4, h, w), (1 << bd) // 3, dt)
    return rec, org


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--depths", default="8,10")
    ap.add_argument("--contents", default="flat,blocky,noise", help="the pick launch is timed on the statistics of the last one")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ctb-log2", type=int, default=6)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    w, h, n, L = a.width, a.height, a.frames, a.ctb_log2
    ctx = deblock.Context(0)
    rows, cols = (h + (1 << L) - 1) >> L, (w + (1 << L) - 1) >> L
    rs = np.random.RandomState(5)
    prm = np.zeros((rows, cols), np.dtype(_lib.SAO_CTB_DTYPE))
    prm["type"] = rs.randint(0, 3, (rows, cols))
    prm["cls"] = np.where(prm["type"] == 1, rs.randint(0, 32, (rows, cols)), rs.randint(0, 4, (rows, cols)))
    prm["offset"] = rs.randint(-7, 8, (rows, cols, 4))
    dp = ctx.alloc(prm.nbytes)
    dp.upload(prm.view(np.uint8).ravel())
    dstats = ctx.alloc(rows * cols * n * 384)
    dpick = ctx.alloc(rows * cols * n * 6)
    lines = []
    for bd in [int(x) for x in a.depths.split(",")]:
        sb = 1 if bd == 8 else 2
        nbytes = 2 * n * w * h * sb
        b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=bd, per_frame_bs=False)
        dorg = ctx.alloc(b.frame_bytes * n)
        p = b.planes()
        res = {}
        for content in a.contents.split(","):
            rec, org = frames_of(content, w, h, bd, np.random.default_rng(11))
            for f in range(n):
                b.upload_frame(f, rec[f % 4])
                dorg.upload(org[(f + 1) % 4], f * b.frame_bytes)
            stats = lambda: ctx.sao_stats_device(p, dorg.ptr, L, out_ptr=dstats.ptr, out_stride=cols, out_frame_stride=rows * cols)
            sao = lambda: ctx.sao_device(p, dp.ptr, cols, L)
            timed(ctx, sao, 100, 0)   # settle the clocks
            ms = {"stats": [], "sao": []}
            for _ in range(a.rounds):
                ms["stats"].append(timed(ctx, stats, a.steps, 10))
                ms["sao"].append(timed(ctx, sao, a.steps, 10))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            res[content] = med["stats"]
            line = {"stage": "sao_stats", "bit_depth": bd, "content": content, "ms_per_call": med, "rounds_ms": ms,
                    "spread_ms": {k: float(max(v) - min(v)) for k, v in ms.items()},
                    "stats_frac_of_8TBps_for_2_planes_read": nbytes / (med["stats"] * 1e-3) / 8e12,
                    "sao_frac_of_8TBps_for_2_planes_moved": nbytes / (med["sao"] * 1e-3) / 8e12, "stats_over_sao": med["stats"] / med["sao"],
                    "workload": "%dx%d %d-bit luma x %d, %d-sample CTBs" % (w, h, bd, n, 1 << L)}
            lines.append(line)
            print(json.dumps(line), flush=True)
        if "flat" in res and "noise" in res:
            line = {"stage": "sao_stats_contention", "bit_depth": bd, "flat_over_noise": res["flat"] / res["noise"]}
            lines.append(line)
            print(json.dumps(line), flush=True)
        pick = lambda: ctx.sao_pick_device(dstats.ptr, cols, cols, rows, bd, 1024, out_ptr=dpick.ptr, out_stride=cols, n_frames=n,
                                           stats_frame_stride=rows * cols, out_frame_stride=rows * cols)
        line = {"stage": "sao_pick", "bit_depth": bd, "ms_per_call": timed(ctx, pick, 20, 5), "ctbs": rows * cols * n, "lambda_q8": 1024,
                "statistics_of": a.contents.split(",")[-1]}
        lines.append(line)
        print(json.dumps(line), flush=True)
        dorg.free()
        b.free()
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
