#!/usr/bin/env python3
"""Random soak of deblocking + SAO of a semi-planar picture in one kernel -- Context.deblock_sao_h265_device(semi_planar=True,
one_kernel=True), i.e. hevcdbk_h265_deblock_sao_device_sp_fused, and, in every third case, Context.deblock_sao_nv12 with a Y plane beside
the pairs -- against tests/sao_sp_ref.py (sp_ref.deblock, then sao) and, for Y, the planar statements of tests/g4_ref.py /
tests/slice_offsets_ref.py.  Each case draws a plane size (multiples of 4 per component, up to three tiles across and two down), a bit
depth of 8 .. 14, square CTBs of 8 / 16 / 32, one QP or a map, the two components' SAO parameters, a keep map or none, a slice / tile
layout or none, per-slice pairs or none and a row pitch on either side of the fused kernels' guard -- on the fused side in two cases of
three, so that with the depths above 12 bit still more than a third of the cases reach the fused kernels.  A case that the guards accept
runs with FUSED_ON (a refusal would raise), every other one with FUSED_AUTO (the two launches).  Every byte is compared, row padding
included.  Prints one JSON line; exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
import g4_ref as G  # noqa: E402
import rext_oracle as rx  # noqa: E402
import sao_borders_ref as B  # noqa: E402
import sao_sp_ref as P  # noqa: E402
import slice_offsets_ref as R  # noqa: E402
import sp_ref as S  # noqa: E402

FILL = 0x5A


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    if a.nbytes:
        d.upload(a.view(np.uint8).ravel())
    return d


def draw(rng, i):
    """the operands of case i"""
    bd = int(rng.choice([8, 8, 9, 10, 10, 12, 13, 14]))
    sb = 1 if bd == 8 else 2
    w, h = 4 * int(rng.integers(2, 60)), 4 * int(rng.integers(2, 44))
    lg = int(rng.choice([3, 4, 5]))
    word, piece = 4 * sb, 16 * sb   # what every kernel needs of a pitch, and what the fused kernels need: a lane's row piece
    pitch = 2 * w * sb + word * int(rng.integers(0, 9))
    if rng.integers(0, 3):
        pitch = -(-pitch // piece) * piece
    elif pitch % piece == 0:
        pitch += word
    c = {"bd": bd, "sb": sb, "w": w, "h": h, "lg": lg, "pitch": pitch, "nv12": i % 3 == 2, "qp": int(rng.integers(24, 46)),
         "frame": S.merge(*[G.blocky_plane(w, h, bd, rng) for _ in range(2)]), "bs": G.random_bs(w, h, rng),
         "qp_map": G.random_qp_map(w, h, 1, S.UNIT_LOG2, rng, lo=26, hi=44) if rng.integers(0, 2) else None,
         "h265": dict(tc_offset_div2=int(rng.integers(-2, 3)), beta_offset_div2=0, cb_qp_offset=int(rng.integers(-6, 7)), cr_qp_offset=int(rng.integers(-6, 7)))}
    pcb, pcr = rx.random_sao_params(w, h, lg, lg, rng, bd), rx.random_sao_params(w, h, lg, lg, rng, bd)
    agree = rng.random(pcb.shape) < 0.7
    pcr["type"] = np.where(agree, pcb["type"], pcr["type"])
    pcr["cls"] = np.where(agree & (pcb["type"] == 2), pcb["cls"], pcr["cls"])
    rows, cols = pcb.shape
    c.update(pcb=pcb, pcr=pcr, keep=G.keep_map(w, h, rng, p=0.2) if rng.integers(0, 2) else None,
             layout=B._layout_of(str(rng.choice(["tiles", "slices", "mixed", "random"])), rows, cols, rng) if rng.integers(0, 2) else None)
    c["pairs"] = None
    if rng.integers(0, 2):
        srows, scols = -(-2 * h >> S.SL_CTB_LOG2), -(-2 * w >> S.SL_CTB_LOG2)
        sidx = R.slices_raster(srows, scols, int(rng.integers(1, 6)))
        c["pairs"] = R.ctb_pairs(sidx, R.table_for(int(sidx.max()) + 1))
    if c["nv12"]:   # a luma plane of twice the size with CTBs twice as large: one CTB grid, one map, one set of slices
        c.update(y=G.blocky_plane(2 * w, 2 * h, bd, rng), ybs=G.random_bs(2 * w, 2 * h, rng, p2=0.4),
                 yprm=rx.random_sao_params(2 * w, 2 * h, lg + 1, lg + 1, rng, bd), ykeep=G.keep_map(2 * w, 2 * h, rng, p=0.2) if rng.integers(0, 2) else None)
    return c


def reference(c):
    """-> (pairs expected, Y expected or None)"""
    h5, bd = c["h265"], c["bd"]
    dbk = S.deblock(c["frame"], *c["bs"], qp=c["qp"], qp_map=c["qp_map"], bit_depth=bd, cb_qp_offset=h5["cb_qp_offset"],
                    cr_qp_offset=h5["cr_qp_offset"], tc_offset_div2=h5["tc_offset_div2"], slice_pairs=c["pairs"])
    want = P.sao(dbk, c["pcb"], c["pcr"], c["lg"], bd, keep=c["keep"], layout=c["layout"])
    if not c["nv12"]:
        return want, None
    from oracle import h265
    vb, hb = c["ybs"]
    if c["pairs"] is not None:
        mid = R.expected(c["y"], vb, hb, c["pairs"], S.SL_CTB_LOG2, c_idx=0, qp=c["qp"], qp_map=c["qp_map"], unit_log2=S.UNIT_LOG2, bit_depth=bd)
    else:
        mid = h265.filter_plane(c["y"], c["qp"], vb, hb, c_idx=0, bit_depth=bd, qp_map=c["qp_map"], unit_log2=S.UNIT_LOG2,
                                tc_offset_div2=h5["tc_offset_div2"], beta_offset_div2=0)
    return want, G.sao_direct(mid, c["yprm"], c["lg"] + 1, c["lg"] + 1, bit_depth=bd, keep=c["ykeep"], layout=c["layout"])


def batch_of(ctx, c, frame, w, h, pitch, bs, semi_planar, free):
    """-> (the batch, its DevicePlanes with the spec-exact mode's bS arrays of the case)"""
    b = deblock.DeviceBatch(ctx, w, h, 1, bit_depth=c["bd"], per_frame_bs=False, pitch=pitch, semi_planar=semi_planar)
    b.upload_all(frame[None], fill=FILL)
    b.dst.upload(np.full(b.frame_bytes // b.sb, FILL, b.dtype))
    if c["qp_map"] is not None:
        b.set_qp_map(c["qp_map"], ctu_log2=S.UNIT_LOG2)
    free += [up(ctx, np.ascontiguousarray(bs[0], np.uint8)), up(ctx, np.ascontiguousarray(bs[1], np.uint8))]
    p = b.planes()   # a luma batch's own arrays are the reference-exact mode's: the 4-sample-granular ones go in here
    p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = free[-2].ptr, free[-1].ptr, 0, 0
    return b, p


def one_case(ctx, rng, i):
    """-> (description, mismatching bytes, took the fused kernels)"""
    c = draw(rng, i)
    want, want_y = reference(c)
    w, h, sb, lg = c["w"], c["h"], c["sb"], c["lg"]
    fusable = c["bd"] <= 12 and c["pitch"] % (16 * sb) == 0   # the guards a draw can miss (dbk_deblock_sao_sp_supports)
    fused = _lib.FUSED_ON if fusable else _lib.FUSED_AUTO
    free = [up(ctx, c["pcb"]), up(ctx, c["pcr"])]
    b, bp = batch_of(ctx, c, c["frame"], w, h, c["pitch"], c["bs"], True, free)
    rows, cols = c["pcb"].shape
    kp = ks = None
    if c["keep"] is not None:
        free.append(up(ctx, c["keep"]))
        kp, ks = free[-1].ptr, c["keep"].shape[1]
    borders = so = None
    if c["layout"] is not None:
        nox = np.ascontiguousarray(B.expected_nox(c["layout"]), np.uint8)
        free.append(up(ctx, nox))
        borders = _lib.SaoBorders(free[-1].ptr, nox.shape[1], 0)
    if c["pairs"] is not None:
        free.append(up(ctx, c["pairs"]))
        so = _lib.SliceOffsets(free[-1].ptr, c["pairs"].shape[1], 0, S.SL_CTB_LOG2)
    yb = None
    if c["nv12"]:
        yb, yp = batch_of(ctx, c, c["y"], 2 * w, 2 * h, None, c["ybs"], False, free)
        free.append(up(ctx, c["yprm"]))
        sl = dict(params=free[-1].ptr, params_stride=c["yprm"].shape[1], ctb_log2=lg + 1)
        if c["ykeep"] is not None:
            free.append(up(ctx, c["ykeep"]))
            sl.update(keep=free[-1].ptr, keep_stride=c["ykeep"].shape[1])
        sp = dict(params_cb=free[0].ptr, params_cr=free[1].ptr, params_stride=cols, ctb_log2=lg, keep=kp, keep_stride=ks or 0)
        ctx.deblock_sao_nv12(yp, bp, c["qp"], sl, sp, h265=c["h265"], fused=fused, borders=borders, slice_offsets=so)
    else:
        ctx.deblock_sao_h265_device(bp, c["qp"], free[0].ptr, cols, lg, keep_ptr=kp, keep_stride=ks or 0, fused=fused, borders=borders,
                                    slice_offsets=so, semi_planar=True, params_cr_ptr=free[1].ptr, one_kernel=True, **c["h265"])
    ctx.synchronize()
    got = b.download_frame(0, with_padding=True)
    bad = int((got[:, : 2 * w].reshape(h, w, 2) != want).sum()) + int((got[:, 2 * w:] != FILL).sum())
    if yb is not None:
        bad += int((yb.download_frame(0) != want_y).sum())
        yb.free()
    b.free()
    for x in free:
        x.free()
    what = "%s %dx%d %d-bit ctb=%d pitch+%d map=%s keep=%s layout=%s slices=%s %s" % (
        "nv12" if c["nv12"] else "sp_fused", w, h, c["bd"], 1 << lg, c["pitch"] - 2 * w * sb, c["qp_map"] is not None, c["keep"] is not None,
        c["layout"] is not None, c["pairs"] is not None, "fused" if fusable else "two launches")
    return what, bad, fusable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0, help="stop after this long (0 = run all cases)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    t0, done, mism, first, fused, kinds = time.time(), 0, 0, None, 0, {}
    for i in range(a.cases):
        what, bad, f = one_case(ctx, rng, i)
        done += 1
        fused += int(f)
        key = what.split()[0] + ", " + ("fused" if f else "two launches")
        kinds[key] = kinds.get(key, 0) + 1
        if bad:
            mism += 1
            first = first or what
        if a.seconds and time.time() - t0 > a.seconds:
            break
    print(json.dumps({"soak": "fused_sp", "seed": a.seed, "cases": done, "by_route": kinds, "fused_share": round(fused / max(done, 1), 3),
                      "mismatching_cases": mism, "first_mismatch": first, "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
