#!/usr/bin/env python3
"""Spec-exact deblocking + SAO of Y, Cb, Cr of F x WxH frames in HBM, src -> dst, in ONE call
(hevcdbk_h265_deblock_sao_device_planes_cf), for a chroma format and bit depth: frames/s and the share of the 8 TB/s HBM peak
with the algorithmic bytes (every sample of the three planes read once and written once).  One QP, bS 2 on every edge,
seeded per-CTB SAO parameters (CtbSizeY 64: 4:2:2 chroma CTBs 32x64), --qp-map: a QP map.  --fused off: the two-launch form, for comparison.
Formats alternate in one process (--chroma-format may be given several times), each measured --repeat times."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_video_codec_amd import deblock, synth, _lib


def setup(ctx, fmt, w, h, n, bd, rng, qp_map_log2=0, qp=32):
    cf = _lib.chroma_format_idc(fmt)
    sx, sy = _lib.CHROMA_SUB[cf]
    L = _lib.lib()
    keep, planes, sao = [], [], []
    for i in range(3):
        pw, ph = (w, h) if i == 0 else (w // sx, h // sy)
        lw, lh = (6, 6) if i == 0 else (6 - (sx - 1), 6 - (sy - 1))
        b = deblock.DeviceBatch(ctx, pw, ph, n, bit_depth=bd, is_chroma=i > 0, per_frame_bs=False)
        src = np.stack([synth.blocky_plane(pw, ph, seed=7 + i, frame=k, bit_depth=bd) for k in range(4)])
        b.upload_all(np.concatenate([src] * (n // 4 + 1))[:n])
        nv, nh = L.hevcdbk_h265_num_vert_bs(pw, ph), L.hevcdbk_h265_num_hor_bs(pw, ph)
        dv, dh = ctx.alloc(nv), ctx.alloc(nh)
        dv.upload(np.full(nv, 2, np.uint8))
        dh.upload(np.full(nh, 2, np.uint8))
        rows, cols = -(-ph >> lh), -(-pw >> lw)
        prm = np.zeros((rows, cols), np.dtype(_lib.SAO_CTB_DTYPE))
        prm["type"] = rng.randint(0, 3, (rows, cols))
        prm["cls"] = np.where(prm["type"] == 1, rng.randint(0, 32, (rows, cols)), rng.randint(0, 4, (rows, cols)))
        prm["offset"] = rng.randint(-7, 8, (rows, cols, 4))
        dp = ctx.alloc(prm.nbytes)
        dp.upload(prm.view(np.uint8).ravel())
        if qp_map_log2:  # one QpY per luma unit, read by every plane at its own positions
            b.set_qp_map(synth.ctu_qp_map(w, h, seed=29, lo=max(qp - 6, 0), hi=min(qp + 6, 51), ctu_log2=qp_map_log2), qp_map_log2)
            keep.append(b.qp_map)
        p = b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
        keep += [b, dv, dh, dp]
        planes.append(p)
        sao.append({"params": dp.ptr, "params_stride": cols, "ctb_log2": lw})
    nbytes = 2 * n * sum(p.plane_w * p.plane_h * p.sample_bytes for p in planes)
    return planes, sao, nbytes, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--bit-depth", type=int, action="append", default=None)
    ap.add_argument("--chroma-format", choices=["420", "422", "444"], action="append", default=None)
    ap.add_argument("--fused", choices=["on", "off"], default="on")
    ap.add_argument("--qp-map", type=int, default=0, metavar="LOG2", help="a QP map of (1 << LOG2)-sample luma units, QP +-6")
    a = ap.parse_args()
    fmts = a.chroma_format or ["420"]
    depths = a.bit_depth or [8]
    ctx = deblock.Context(0)
    fused = _lib.FUSED_ON if a.fused == "on" else _lib.FUSED_OFF
    h265 = {"tc_offset_div2": 0, "beta_offset_div2": 0, "cb_qp_offset": 0, "cr_qp_offset": 0}
    cfgs = [(f, bd) for bd in depths for f in fmts]
    res = {"%s_%dbit" % c: [] for c in cfgs}
    for _ in range(a.repeat):
        for fmt, bd in cfgs:
            planes, sao, nbytes, keep = setup(ctx, fmt, a.width, a.height, a.frames, bd, np.random.RandomState(5), a.qp_map, a.qp)
            call = lambda: ctx.deblock_sao_device_planes(planes, a.qp, sao, h265=h265, fused=fused, chroma_format=fmt)
            for _ in range(max(a.steps, 50)):
                call()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call()
            ctx.synchronize()
            dt = (time.perf_counter() - t0) / a.steps
            res["%s_%dbit" % (fmt, bd)].append({"ms_per_step": round(dt * 1e3, 4), "frac_of_8TBps": round(nbytes / dt / 8e12, 4)})
            for x in keep:
                x.free()
    print(json.dumps({"stage": "spec-exact deblock+sao, Y+Cb+Cr in one call", "fused": a.fused,
                      "workload": "%dx%d x %d frames, QP %d%s, bS 2 everywhere, CtbSizeY 64" % (
                          a.width, a.height, a.frames, a.qp, " +-6 per %d-sample unit" % (1 << a.qp_map) if a.qp_map else ""),
                      "results": res}))


if __name__ == "__main__":
    main()
