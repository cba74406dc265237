#!/usr/bin/env python3
"""SAO statistics pass (hevcdbk_sao_stats_device) rate: 64 x 3840x2160 luma in HBM at 8 and 10 bit, on noise, on a blocky picture
and on a flat one (every sample in ONE band bin and in no edge bin: what contention on a bin costs).  The statistics launch and the
existing SAO pass (the leg of tools/bench_sao.py: seeded per-CTB parameters, one third off / band / edge) take turns in this one
process on the same planes; both move two planes' worth of bytes -- the statistics pass reads two, SAO reads one and writes one.
Wall clock over back-to-back launches that end in a synchronise; the median over the rounds is reported, and the spread between
them.  The pick launch is timed once per depth, for the record.  One JSON line per (depth, content).  Diagnostic.

--semi-planar: the statistics of a plane of interleaved Cb / Cr pairs (960x540 and 1920x1080 pairs, 64 frames, 32-sample CTBs, noise
and flat) in three forms that take turns on the same buffers: (a) one hevcdbk_sao_stats_device_sp launch; (b) two
hevcdbk_sao_stats_device launches on planes that are already split; (c) as (b) after the two strided copies that split rec and the
two that split org (torch, on the stream the launches use).  Every form fills the same two arrays, compared once per row.

--decide: the decision per CTB (hevcdbk_sao_decide_device: own parameters, merge left or merge up over Y, Cb and Cr) for 64 frames of
3840x2160 at 64- and 16-sample CTBs, taking turns with the luma statistics pass and the two pick launches on the same batch -- and
with the _os entries (log2_sao_offset_scale, the candidates compared by a wave's lanes together) at a scale of 0, where they write the
same bytes.

--slice-flags: hevcdbk_sao_slice_flags_device (slice_sao_luma_flag / slice_sao_chroma_flag chosen per slice, and the decision under
them) against hevcdbk_sao_decide_device_os on the same arrays, taking turns, at 64- and 16-sample CTBs with the frame in 8 and in 135
slices of whole CTB rows.  The yardstick is THREE _os decisions: what a caller had to run before summing on the host."""
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


def semi_planar(a):
    import torch
    ctx = deblock.Context(0)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)            # one stream of its own for the copies and the launches: the default stream's handle is 0,
    torch.cuda.set_stream(side)              # which the entries read as "the context's compute stream"
    stream = side.cuda_stream
    assert stream
    n, L = a.frames, 5
    lines = []
    for (w, h) in [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")]:
        rows, cols = (h + 31) >> L, (w + 31) >> L
        g = rows * cols
        for bd in [int(x) for x in a.depths.split(",")]:
            sb = 1 if bd == 8 else 2
            tdt, ndt = (torch.uint8, np.uint8) if sb == 1 else (torch.int16, np.uint16)
            for content in a.contents.split(","):
                rng = np.random.default_rng(11)
                org = rng.integers(0, 1 << bd, (4, h, w, 2)).astype(ndt)
                rec = rng.integers(0, 1 << bd, (4, h, w, 2)).astype(ndt) if content == "noise" else np.full((4, h, w, 2), (1 << bd) // 3, ndt)
                frames = lambda x: torch.from_numpy(x.view(np.uint8 if sb == 1 else np.int16)).to(dev).repeat(n // 4 + 1, 1, 1, 1)[:n].contiguous()
                t_rec, t_org = frames(rec), frames(np.roll(org, 1, axis=0))                     # (n, h, w, 2) pairs
                split = [torch.empty((n, h, w), dtype=tdt, device=dev) for _ in range(4)]       # rec Cb, rec Cr, org Cb, org Cr
                st = [torch.zeros((n * g, 96), dtype=torch.int32, device=dev) for _ in range(2)]

                def planes(t, pitch_samples, chroma):
                    p = _lib.DevicePlanes()
                    p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = t.data_ptr(), 0, pitch_samples * sb, pitch_samples * h * sb, n
                    p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = w, h, bd, sb, chroma
                    return p
                psp, pcb, pcr = planes(t_rec, 2 * w, 1), planes(split[0], w, 1), planes(split[1], w, 1)

                def form_a():
                    ctx.sao_stats_device(psp, t_org.data_ptr(), L, out_ptr=st[0].data_ptr(), out_cr_ptr=st[1].data_ptr(), out_stride=cols,
                                         out_frame_stride=g, stream=stream, semi_planar=True)

                def form_b():
                    for c, p in enumerate((pcb, pcr)):
                        ctx.sao_stats_device(p, split[2 + c].data_ptr(), L, ctb_log2_h=L, out_ptr=st[c].data_ptr(), out_stride=cols, out_frame_stride=g,
                                             stream=stream)

                def copies():
                    for c in (0, 1):
                        split[c].copy_(t_rec[..., c])
                        split[2 + c].copy_(t_org[..., c])

                def form_c():
                    copies()
                    form_b()
                forms = {"a_sp": form_a, "b_two_planar": form_b, "c_split_and_two_planar": form_c}
                results = {}
                for k in ("c_split_and_two_planar", "a_sp"):                                    # c first: it fills the split planes
                    for t in st:
                        t.fill_(-1)
                    forms[k]()
                    torch.cuda.synchronize(dev)
                    results[k] = [t.cpu().numpy().copy() for t in st]
                same = all(np.array_equal(x, y) for x, y in zip(results["a_sp"], results["c_split_and_two_planar"]))
                sync = lambda: torch.cuda.synchronize(dev)

                def timed_t(fn, steps, warm):
                    for _ in range(warm):
                        fn()
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        fn()
                    sync()
                    return (time.perf_counter() - t0) / steps * 1e3
                timed_t(form_c, 60, 0)   # settle the clocks
                ms = {k: [] for k in forms}
                for _ in range(a.rounds):
                    for k, fn in forms.items():
                        ms[k].append(timed_t(fn, a.steps, 10))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
                nbytes = 4 * n * w * h * sb                                                     # two pair planes read
                line = {"stage": "sao_stats_sp", "pairs": "%dx%d" % (w, h), "bit_depth": bd, "content": content, "frames": n, "ctb": 1 << L,
                        "ms_per_call": med, "rounds_ms": ms, "spread_ms": spread, "outputs_identical": bool(same),
                        "a_over_b": med["a_sp"] / med["b_two_planar"], "c_over_a": med["c_split_and_two_planar"] / med["a_sp"],
                        "a_loses_to_b_beyond_spread": bool(med["a_sp"] - med["b_two_planar"] > max(spread["a_sp"], spread["b_two_planar"])),
                        "a_frac_of_8TBps_for_2_pair_planes_read": nbytes / (med["a_sp"] * 1e-3) / 8e12}
                lines.append(line)
                print(json.dumps(line), flush=True)
                del t_rec, t_org, split, st
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def decide(a):
    """--decide: hevcdbk_sao_decide_device (Y, Cb, Cr on one CTB grid) on a.frames frames of a.width x a.height at each CTB size of
    a.ctbs, taking turns in this process with the luma statistics pass and with the two pick launches (luma alone, Cb and Cr jointly)
    that produce what the decision's NEW candidates are, and with the _os forms of both at a scale of 0 -- on the same batch.  The three statistics arrays are those of the luma
    plane against three different originals: real statistics, one record per CTB.  One JSON line per CTB size."""
    w, h, n, bd, lam = a.width, a.height, a.frames, 8, 1024
    ctx = deblock.Context(0)
    b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=bd, per_frame_bs=False)
    dorg = ctx.alloc(b.frame_bytes * (n + 2))
    rec, org = frames_of("blocky", w, h, bd, np.random.default_rng(11))
    for f in range(n + 2):
        if f < n:
            b.upload_frame(f, rec[f % 4])
        dorg.upload(org[(f + 1) % 4], f * b.frame_bytes)
    p = b.planes()
    lines = []
    for L in [int(x) for x in a.ctbs.split(",")]:
        rows, cols = (h + (1 << L) - 1) >> L, (w + (1 << L) - 1) >> L
        g = rows * cols
        dst = [ctx.alloc(g * n * 384) for _ in range(3)]
        dprm = [ctx.alloc(g * n * 6) for _ in range(3)]
        ddec = ctx.alloc(g * n * 32)
        stats = lambda c=0: ctx.sao_stats_device(p, dorg.ptr + c * b.frame_bytes, L, out_ptr=dst[c].ptr, out_stride=cols, out_frame_stride=g)
        for c in range(3):
            stats(c)

        def picks(scale=None):
            ctx.sao_pick_device(dst[0].ptr, cols, cols, rows, bd, lam, out_ptr=dprm[0].ptr, out_stride=cols, n_frames=n, stats_frame_stride=g,
                                out_frame_stride=g, log2_offset_scale=scale)
            ctx.sao_pick_device(dst[1].ptr, cols, cols, rows, bd, lam, out_ptr=dprm[1].ptr, out_stride=cols, n_frames=n, stats_frame_stride=g,
                                out_frame_stride=g, stats_b_ptr=dst[2].ptr, out_b_ptr=dprm[2].ptr, log2_offset_scale=scale)

        def dec(scale=None):
            ctx.sao_decide_device(dst[0].ptr, cols, cols, rows, bd, lam, out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr,
                                  decision_stride=cols, n_frames=n, stats_frame_stride=g, out_frame_stride=g, decision_frame_stride=g,
                                  stats_cb_ptr=dst[1].ptr, stats_cr_ptr=dst[2].ptr, out_cb_ptr=dprm[1].ptr, out_cr_ptr=dprm[2].ptr,
                                  log2_offset_scale=scale)
        # the _os entries at a scale of 0 write what the entries without a scale write: compared once, before the turns
        outputs = {}
        for k, fn in (("decide", dec), ("decide_os", lambda: dec(0)), ("two_picks", picks), ("two_picks_os", lambda: picks(0))):
            fn()
            ctx.synchronize()
            outputs[k] = [d.download(g * n * 6).tobytes() for d in dprm] + ([ddec.download(g * n * 32).tobytes()] if k.startswith("decide") else [])
        forms = {"stats_luma": stats, "two_picks": picks, "two_picks_os": lambda: picks(0), "decide": dec, "decide_os": lambda: dec(0)}
        timed(ctx, stats, 30, 0)   # settle the clocks
        ms = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():
                ms[k].append(timed(ctx, fn, a.steps, 5))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        dec()
        ctx.synchronize()
        merge = np.bincount(ddec.download(g * n * 32).view(np.dtype(_lib.SAO_DECISION_DTYPE))["merge"], minlength=3)
        spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
        slower = lambda new, old: bool(med[new] - med[old] > max(spread[new], spread[old]))
        line = {"stage": "sao_decide", "workload": "%dx%d %d-bit x %d, %d-sample CTBs, Y + Cb + Cr on one grid" % (w, h, bd, n, 1 << L),
                "ctbs": g * n, "lambda_q8": lam, "ms_per_call": med, "rounds_ms": ms, "spread_ms": spread,
                "decide_over_stats_luma": med["decide"] / med["stats_luma"], "decide_over_two_picks": med["decide"] / med["two_picks"],
                "decide_slower_than_stats_luma": bool(med["decide"] > med["stats_luma"]), "merge_0_left_up": [int(x) for x in merge],
                "decide_os_over_decide": med["decide_os"] / med["decide"], "two_picks_os_over_two_picks": med["two_picks_os"] / med["two_picks"],
                "decide_os_over_stats_luma": med["decide_os"] / med["stats_luma"],
                "decide_os_slower_than_decide_beyond_spread": slower("decide_os", "decide"),
                "two_picks_os_slower_than_two_picks_beyond_spread": slower("two_picks_os", "two_picks"),
                "os_outputs_identical_at_scale_0": bool(outputs["decide"] == outputs["decide_os"] and outputs["two_picks"] == outputs["two_picks_os"])}
        lines.append(line)
        print(json.dumps(line), flush=True)
        for d in dst + dprm + [ddec]:
            d.free()
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def slice_flags(a):
    """--slice-flags: one JSON line per (CTB size, slices per frame); the statistics arrays are those of --decide"""
    w, h, n, bd, lam = a.width, a.height, a.frames, 8, 1024
    ctx = deblock.Context(0)
    b = deblock.DeviceBatch(ctx, w, h, n, bit_depth=bd, per_frame_bs=False)
    dorg = ctx.alloc(b.frame_bytes * (n + 2))
    rec, org = frames_of("blocky", w, h, bd, np.random.default_rng(11))
    for f in range(n + 2):
        if f < n:
            b.upload_frame(f, rec[f % 4])
        dorg.upload(org[(f + 1) % 4], f * b.frame_bytes)
    p = b.planes()
    lines = []
    for L in [int(x) for x in a.ctbs.split(",")]:
        rows, cols = (h + (1 << L) - 1) >> L, (w + (1 << L) - 1) >> L
        g = rows * cols
        dst = [ctx.alloc(g * n * 384) for _ in range(3)]
        dprm = [ctx.alloc(g * n * 6) for _ in range(3)]
        ddec = ctx.alloc(g * n * 32)
        for c in range(3):
            ctx.sao_stats_device(p, dorg.ptr + c * b.frame_bytes, L, out_ptr=dst[c].ptr, out_stride=cols, out_frame_stride=g)
        need = ctx.sao_slice_flags_workspace(cols, rows, n, 600)
        dws = ctx.alloc(need)
        for n_slices in [int(x) for x in a.slices.split(",")]:
            sl = (np.arange(rows)[:, None] * min(n_slices, rows) // rows + np.zeros((1, cols), np.int64)).astype(np.uint16)
            dsl = ctx.alloc(sl.nbytes)
            dsl.upload(sl.view(np.uint8).ravel())
            dfl, dsr = ctx.alloc(n * n_slices), ctx.alloc(n * n_slices * 72)
            common = dict(out_ptr=dprm[0].ptr, out_stride=cols, decision_ptr=ddec.ptr, decision_stride=cols, n_frames=n, stats_frame_stride=g,
                          out_frame_stride=g, decision_frame_stride=g, stats_cb_ptr=dst[1].ptr, stats_cr_ptr=dst[2].ptr, out_cb_ptr=dprm[1].ptr,
                          out_cr_ptr=dprm[2].ptr, slice_idx_ptr=dsl.ptr, idx_stride=cols, idx_frame_stride=0)

            def dec_os():
                ctx.sao_decide_device(dst[0].ptr, cols, cols, rows, bd, lam, log2_offset_scale=0, **common)

            def three():
                for _ in range(3):
                    dec_os()

            def choose():
                ctx.sao_slice_flags_device(dst[0].ptr, cols, cols, rows, bd, lam, n_slices=n_slices, slice_flags_ptr=dfl.ptr,
                                           slice_flags_frame_stride=n_slices, slice_record_ptr=dsr.ptr, slice_record_frame_stride=n_slices,
                                           workspace_ptr=dws.ptr, workspace_bytes=need, **common)
            forms = {"decide_os": dec_os, "three_decide_os": three, "slice_flags": choose}
            timed(ctx, dec_os, 30, 0)   # settle the clocks
            ms = {k: [] for k in forms}
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    ms[k].append(timed(ctx, fn, a.steps, 5))
            med = {k: float(np.median(v)) for k, v in ms.items()}
            spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
            choose()
            ctx.synchronize()
            chosen = np.bincount(dfl.download(n * n_slices), minlength=4)
            line = {"stage": "sao_slice_flags", "workload": "%dx%d %d-bit x %d, %d-sample CTBs, Y + Cb + Cr on one grid, %d slices per frame"
                    % (w, h, bd, n, 1 << L, n_slices), "ctbs": g * n, "lambda_q8": lam, "workspace_bytes": need, "ms_per_call": med, "rounds_ms": ms,
                    "spread_ms": spread, "slice_flags_over_decide_os": med["slice_flags"] / med["decide_os"],
                    "slice_flags_over_three_decide_os": med["slice_flags"] / med["three_decide_os"],
                    "slice_flags_slower_than_three_decide_os": bool(med["slice_flags"] > med["three_decide_os"]),
                    "slices_per_pair_0_1_2_3": [int(x) for x in chosen]}
            lines.append(line)
            print(json.dumps(line), flush=True)
            for d in (dsl, dfl, dsr):
                d.free()
        for d in dst + dprm + [ddec, dws]:
            d.free()
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slice-flags", action="store_true", help="the slice-level flags chosen on the device against one and three _os decisions")
    ap.add_argument("--slices", default="8,135", help="--slice-flags: slices per frame (whole CTB rows)")
    ap.add_argument("--decide", action="store_true", help="the decision per CTB against the luma statistics pass and the two pick launches")
    ap.add_argument("--ctbs", default="6,4", help="--decide: log2 of the CTB sizes")
    ap.add_argument("--semi-planar", action="store_true", help="the pair-plane entry against two planar launches, with and without the split copies")
    ap.add_argument("--sizes", default="960x540,1920x1080", help="--semi-planar: pairs per row x rows")
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
    if a.decide:
        return decide(a)
    if a.slice_flags:
        return slice_flags(a)
    if a.semi_planar:
        if a.contents == "flat,blocky,noise":
            a.contents = "noise,flat"
        return semi_planar(a)
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
