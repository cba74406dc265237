#!/usr/bin/env python3
"""Measured distortion (hevcdbk_sse_device, hevcdbk_sse_device_sp, hevcdbk_sse_totals_device) rate: 64 x 3840x2160 luma and
64 x 1920x1080 pairs in HBM at 8 and 10 bit, CTBs of 64 and 16 samples (32 and 8 for the pairs).  Each entry takes turns in this one
process, on the same planes, with the unchanged statistics pass (hevcdbk_sao_stats_device / _sp), with the SAO pass (seeded per-CTB
parameters, one third off / band / edge) and with a plain device-to-device copy of ONE plane -- which moves the bytes the SSE pass
reads (two planes' worth): the copy floor.  Wall clock over back-to-back launches that end in a synchronise, after a warm-up; the
median over the rounds is reported and the spread between them.  The SSE entry is also timed on the same planes one quad of samples
further on -- rows at a multiple of four samples but not of 16 bytes: the four-samples-per-load path, which at 8 bit is also the
64-sample-wide region against the 128-sample-wide one -- and one sample further on (sample by sample).  One JSON line per (plane
kind, depth, CTB size).  Diagnostic."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import deblock, _lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--depths", default="8,10")
    ap.add_argument("--kinds", default="luma,pairs")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    import torch
    ctx = deblock.Context(0)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)            # a stream of its own for the copies and the launches: the default stream's handle is 0,
    torch.cuda.set_stream(side)              # which the entries read as "the context's compute stream"
    stream = side.cuda_stream
    assert stream
    n = a.frames
    sync = lambda: torch.cuda.synchronize(dev)

    def timed(fn, steps, warm):
        for _ in range(warm):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        sync()
        return (time.perf_counter() - t0) / steps * 1e3

    lines = []
    for kind in a.kinds.split(","):
        pairs = kind == "pairs"
        w, h = (1920, 1080) if pairs else (3840, 2160)
        row = 2 * w if pairs else w
        for bd in [int(x) for x in a.depths.split(",")]:
            sb = 1 if bd == 8 else 2
            tdt, ndt = (torch.uint8, np.uint8) if sb == 1 else (torch.int16, np.uint16)
            rng = np.random.default_rng(11)
            slack = 16 // sb                                           # room to move a plane on by a quad or by a sample
            def frames():
                x = rng.integers(0, 1 << bd, (4, h, row)).astype(ndt)
                t = torch.from_numpy(x.view(np.uint8 if sb == 1 else np.int16)).to(dev).repeat(n // 4 + 1, 1, 1)[:n].reshape(-1)
                return torch.cat([t, torch.zeros(slack, dtype=tdt, device=dev)])
            t_rec, t_org = frames(), frames()
            t_dst = torch.empty_like(t_rec)

            def planes(off=0):
                p = _lib.DevicePlanes()
                p.src, p.dst, p.pitch, p.frame_stride, p.n_frames = t_rec.data_ptr() + off * sb, t_dst.data_ptr() + off * sb, row * sb, row * h * sb, n
                p.plane_w, p.plane_h, p.bit_depth, p.sample_bytes, p.is_chroma = w, h, bd, sb, int(pairs)
                return p
            for L in ((5, 3) if pairs else (6, 4)):
                rows, cols = (h + (1 << L) - 1) >> L, (w + (1 << L) - 1) >> L
                g = rows * cols
                rs = np.random.RandomState(5)
                prm = np.zeros((rows, cols), np.dtype(_lib.SAO_CTB_DTYPE))
                prm["type"] = rs.randint(0, 3, (rows, cols))
                prm["cls"] = np.where(prm["type"] == 1, rs.randint(0, 32, (rows, cols)), rs.randint(0, 4, (rows, cols)))
                prm["offset"] = rs.randint(-7, 8, (rows, cols, 4))
                t_prm = torch.from_numpy(prm.view(np.uint8).reshape(-1).copy()).to(dev)
                t_stats = [torch.zeros((n * g, 96), dtype=torch.int32, device=dev) for _ in range(2)]
                t_sse = [torch.zeros(n * g, dtype=torch.int64, device=dev) for _ in range(2)]
                t_tot, t_ft = torch.zeros(n * 600, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
                sl = (np.arange(rows)[:, None] * min(8, rows) // rows + np.zeros((1, cols), np.int64)).astype(np.int16)
                t_sl = torch.from_numpy(sl).to(dev)
                sp = dict(semi_planar=True) if pairs else {}

                def sse(off=0):
                    ctx.sse_device(planes(off), t_org.data_ptr() + off * sb, L, out_ptr=t_sse[0].data_ptr(), out_stride=cols, out_frame_stride=g,
                                   stream=stream, **(dict(sp, out_cr_ptr=t_sse[1].data_ptr()) if pairs else {}))

                def stats():
                    ctx.sao_stats_device(planes(), t_org.data_ptr(), L, out_ptr=t_stats[0].data_ptr(), out_stride=cols, out_frame_stride=g,
                                         stream=stream, **(dict(sp, out_cr_ptr=t_stats[1].data_ptr()) if pairs else {}))

                def sao():
                    ctx.sao_device(planes(), t_prm.data_ptr(), cols, L, **(dict(sp, params_cr_ptr=t_prm.data_ptr()) if pairs else dict(g4=True)))

                def copy():
                    t_dst.copy_(t_rec)

                def totals(ns):
                    ctx.sse_totals_device(t_sse[0].data_ptr(), cols, cols, rows, n_frames=n, sse_frame_stride=g, slice_idx_ptr=t_sl.data_ptr(),
                                          idx_stride=cols, n_slices=ns, slice_total_ptr=t_tot.data_ptr(), slice_total_frame_stride=600,
                                          frame_total_ptr=t_ft.data_ptr(), stream=stream)
                forms = {"sse": sse, "sse_quads": lambda: sse(4), "sse_samples": lambda: sse(1), "stats": stats, "sao": sao, "copy_one_plane": copy,
                         "totals_8_slices": lambda: totals(8), "totals_600_slices": lambda: totals(600)}
                # the three load paths fill the same array where the planes are the same: compared once on the path every later row times
                sse()
                sync()
                first = [t.cpu().numpy().copy() for t in t_sse]
                ctx.synchronize()
                timed(copy, 30, 0)   # settle the clocks
                ms = {k: [] for k in forms}
                for _ in range(a.rounds):
                    for k, fn in forms.items():
                        ms[k].append(timed(fn, a.steps, 5))
                sse()
                sync()
                same = all(np.array_equal(x, t.cpu().numpy()) for x, t in zip(first, t_sse))
                med = {k: float(np.median(v)) for k, v in ms.items()}
                spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
                nbytes = 2 * n * row * h * sb + (2 if pairs else 1) * n * g * 8                # two planes read, the outputs written
                line = {"stage": "sse_sp" if pairs else "sse", "workload": "%dx%d %s, %d-bit x %d, %d-sample CTBs" % (w, h, kind, bd, n, 1 << L),
                        "bit_depth": bd, "ctb": 1 << L, "ms_per_call": med, "spread_ms": spread, "rounds_ms": ms,
                        "algorithmic_bytes": nbytes, "sse_frac_of_8TBps": nbytes / (med["sse"] * 1e-3) / 8e12,
                        "copy_frac_of_8TBps_for_one_plane_read_and_written": 2 * n * row * h * sb / (med["copy_one_plane"] * 1e-3) / 8e12,
                        "sse_over_stats": med["sse"] / med["stats"], "sse_over_sao": med["sse"] / med["sao"], "sse_over_copy": med["sse"] / med["copy_one_plane"],
                        "sse_slower_than_stats": bool(med["sse"] > med["stats"]),
                        "sse_slower_than_copy_beyond_spread": bool(med["sse"] - med["copy_one_plane"] > max(spread["sse"], spread["copy_one_plane"])),
                        "same_bits_after_the_rounds": bool(same)}
                lines.append(line)
                print(json.dumps(line), flush=True)
            del t_rec, t_org, t_dst
    if a.out:
        with open(a.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
