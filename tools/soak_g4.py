#!/usr/bin/env python3
"""Random soak of the _g4 entries (planes sized in multiples of 4, not 8: the 960x540 chroma planes of a 1920x1080 picture) against
tests/g4_ref.py: each case draws a chroma format, a g4 chroma plane size, a bit depth, a CTB size, one QP or a QP map, bS arrays with
keep flags, per-slice offsets or none, slice / tile borders or none, a keep map or none, a row pitch, and an entry --
  deblocking only (32-bit / packed kernel with either block-to-lane map / automatic, in place or not),
  SAO only,
  deblocking + SAO of the plane (fused AUTO / ON / OFF),
  deblocking + SAO of Y + Cb + Cr of the picture in one call (4:2:0 and 4:2:2, whose luma plane is a multiple of 8)
-- runs it on device 0 and compares every byte.  Prints one JSON line; exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
import g4_ref as G  # noqa: E402
import rext_oracle as rx  # noqa: E402
import sao_borders_ref as B  # noqa: E402
import slice_offsets_ref as R  # noqa: E402


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    if a.nbytes:
        d.upload(a.view(np.uint8).ravel())
    return d


def plane_of(ctx, rng, w, h, bd, chroma, frame, vb, hb, qmap, u, free, in_place=False):
    """a one-frame batch with a random row pitch, its bS arrays and QP map -> (batch, planes)"""
    sb = 1 if bd == 8 else 2
    pitch = w * sb + 8 * int(rng.integers(0, 4)) + (4 if sb == 1 and rng.integers(0, 2) else 0)
    b = deblock.DeviceBatch(ctx, w, h, 1, bit_depth=bd, is_chroma=chroma, per_frame_bs=False, pitch=pitch, in_place=in_place)
    b.upload_all(frame[None], fill=0x5A)
    p = b.planes()
    if vb is not None:
        dv, dh = up(ctx, vb), up(ctx, hb)
        free += [dv, dh]
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
    if qmap is not None:
        b.set_qp_map(qmap, u)
        p.qp_map, p.qp_map_stride, p.ctu_log2, p.qp_map_frame_stride = b.qp_map.ptr, b.map_stride, b.ctu_log2, b.map_frame_stride
    return b, p


def one_case(ctx, rng):
    """-> (description, mismatching bytes, samples changed at the new last edges, samples of the last row / column that padding would
    have got wrong)"""
    kind = str(rng.choice(["dbk", "sao", "both", "picture"]))
    cf = int(rng.choice([1, 2] if kind == "picture" else [1, 2, 3]))
    sx, sy = rx.SUB[cf]
    bd = int(rng.choice([8, 10, 12]))
    while True:
        w, h = 4 * int(rng.integers(2, 80)), 4 * int(rng.integers(2, 40))
        if kind == "picture" and ((w * sx) % 8 or (h * sy) % 8):
            continue
        if G.is_g4(w, h):
            break
    ctb_y = int(rng.choice([4, 5, 6]))
    lw, lh = ctb_y - (sx - 1), ctb_y - (sy - 1)
    u = int(rng.choice([3, 4, 6]))
    qmap = rng.integers(18, 52, (-(-h * sy >> u), -(-w * sx >> u))).astype(np.uint8) if rng.integers(0, 2) else None
    qp = int(rng.integers(18, 52))
    hp = dict(tc_offset_div2=int(rng.integers(-6, 7)), beta_offset_div2=int(rng.integers(-6, 7)), cb_qp_offset=int(rng.integers(-4, 5)),
              cr_qp_offset=int(rng.integers(-4, 5)))
    free, batches, want = [], [], []
    edge = pad_diff = 0
    # per-slice offsets on the luma CTB grid, slice / tile borders on the plane's own CTB grid (= the luma grid sub-sampled)
    rows, cols = -(-h * sy >> ctb_y), -(-w * sx >> ctb_y)
    so = pairs = None
    if kind != "sao" and rng.integers(0, 2):
        sidx = R.slices_raster(rows, cols, int(rng.integers(1, rows * cols + 1)))
        pairs = R.ctb_pairs(sidx, rng.integers(-6, 7, (int(sidx.max()) + 1, 2)).astype(np.int8))
        dso = up(ctx, pairs)
        free.append(dso)
        so = _lib.SliceOffsets(dso.ptr, cols, 0, ctb_y)
    bo = lay = None
    if kind != "dbk" and rng.integers(0, 2):
        lay = B._layout_of(str(rng.choice(["tiles", "slices", "mixed", "random"])), rows, cols, rng)
        dbo = up(ctx, B.expected_nox(lay))
        free.append(dbo)
        bo = _lib.SaoBorders(dbo.ptr, cols, 0)
    fused = int(rng.choice([_lib.FUSED_AUTO, _lib.FUSED_ON, _lib.FUSED_OFF]))
    variant = int(rng.choice([_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED, _lib.KERNEL_PACKED | _lib.MAP_LINEAR,
                              _lib.KERNEL_PACKED | _lib.MAP_ROWS]))
    in_place = kind == "dbk" and bool(rng.integers(0, 2))

    def deblocked(frame, vb, hb, c_idx):
        cq = 0 if c_idx == 0 else (hp["cb_qp_offset"] if c_idx == 1 else hp["cr_qp_offset"])
        kw = dict(qp=qp, qp_map=qmap, unit_log2=u, bit_depth=bd)
        if c_idx == 0:
            from oracle import h265
            if pairs is not None:
                return R.expected(frame, vb, hb, pairs, ctb_y, c_idx=0, **kw)
            return h265.filter_plane(frame, qp, vb, hb, c_idx=0, bit_depth=bd, qp_map=qmap, unit_log2=u,
                                     tc_offset_div2=hp["tc_offset_div2"], beta_offset_div2=hp["beta_offset_div2"])
        if pairs is not None:
            return G.deblock_sl(frame, vb, hb, cf, pairs, ctb_y, c_qp_offset=cq, **kw)
        return G.deblock_direct(frame, vb, hb, cf, c_qp_offset=cq, tc_offset_div2=hp["tc_offset_div2"], **kw)

    def sao_of(mid, pw, ph, plw, plh):
        nonlocal pad_diff
        prm = G.border_params(pw, ph, plw, plh, bd, 1, rng)[0] if rng.integers(0, 2) else rx.random_sao_params(pw, ph, plw, plh, rng, bd)
        keep = G.keep_map(pw, ph, rng) if rng.integers(0, 2) else None
        dp = up(ctx, prm)
        free.append(dp)
        d = {"params": dp.ptr, "params_stride": prm.shape[1], "ctb_log2": plw, "ctb_log2_h": plh}
        if keep is not None:
            dk = up(ctx, keep)
            free.append(dk)
            d.update(keep=dk.ptr, keep_stride=keep.shape[1])
        out = G.sao_direct(mid, prm, plw, plh, bit_depth=bd, keep=keep, layout=lay)
        if G.is_g4(pw, ph) and lay is None and keep is None:
            pad_diff += int((G.padded_sao(mid, prm, plw, plh, bit_depth=bd) != out).sum())
        return d, out

    planes, saos = [], []
    idx = [0, 1, 2] if kind == "picture" else [int(rng.integers(1, 3))]
    lvb = lhb = None
    if kind == "picture":
        lvb, lhb = G.random_bs(w * sx, h * sy, rng, p2=0.4)
    for i in idx:
        pw, ph = (w * sx, h * sy) if i == 0 else (w, h)
        plw, plh = (ctb_y, ctb_y) if i == 0 else (lw, lh)
        frame = G.blocky_plane(pw, ph, bd, rng) if rng.integers(0, 4) else G.noise_plane(pw, ph, bd, rng)
        if kind == "sao":
            vb = hb = None
        elif kind == "picture":
            vb, hb = (lvb, lhb) if i == 0 else rx.chroma_bs(lvb, lhb, w * sx, h * sy, cf)
        else:
            vb, hb = G.random_bs(pw, ph, rng)
        b, p = plane_of(ctx, rng, pw, ph, bd, i > 0, frame, vb, hb, qmap if kind != "sao" else None, u, free, in_place)
        batches.append(b)
        planes.append(p)
        mid = frame if kind == "sao" else deblocked(frame, vb, hb, i)
        if kind != "sao" and i > 0:
            edge += sum(G.new_edge_changes(frame, mid))
        if kind == "dbk":
            want.append(mid)
        else:
            d, out = sao_of(mid, pw, ph, plw, plh)
            saos.append(d)
            want.append(out)

    def retry(call, selector_forced):
        try:
            call(False)
        except deblock.DeblockError as e:   # operands a kernel family does not take, with a g4 plane as with a multiple of 8
            if e.code != _lib.ERR_UNSUPPORTED or not selector_forced:
                raise
            call(True)

    c_idx = idx[0]
    if kind == "dbk":
        retry(lambda auto: ctx.filter_device_h265(planes[0], qp, c_idx=c_idx, chroma_format=str(_fmt(cf)), slice_offsets=so, g4=True,
                                                  variant=_lib.KERNEL_AUTO if auto else variant, **hp), (variant & 0xff) == _lib.KERNEL_PACKED)
    elif kind == "sao":
        d = saos[0]
        ctx.sao_device(planes[0], d["params"], d["params_stride"], lw, keep_ptr=d.get("keep"), keep_stride=d.get("keep_stride", 0),
                       chroma_format=str(_fmt(cf)), ctb_log2_h=lh, borders=bo, g4=True)
    elif kind == "both":
        d = saos[0]
        retry(lambda auto: ctx.deblock_sao_h265_device(planes[0], qp, d["params"], d["params_stride"], lw, c_idx=c_idx, keep_ptr=d.get("keep"),
                                                       keep_stride=d.get("keep_stride", 0), fused=_lib.FUSED_AUTO if auto else fused,
                                                       chroma_format=str(_fmt(cf)), ctb_log2_h=lh, borders=bo, slice_offsets=so, g4=True, **hp),
              fused == _lib.FUSED_ON)
    else:
        retry(lambda auto: ctx.deblock_sao_device_planes(planes, qp, saos, h265=hp, fused=_lib.FUSED_AUTO if auto else fused,
                                                         chroma_format=str(_fmt(cf)), borders=bo, slice_offsets=so, g4=True), fused == _lib.FUSED_ON)
    ctx.synchronize()
    bad = 0
    for i, b in enumerate(batches):
        got = b.download_frame(0, with_padding=True)
        bad += int((got[:, : b.w] != want[i]).sum())
        if b.qp_map is not None:
            b.qp_map.free()
        b.free()
    for x in free:
        x.free()
    what = "%s 4:%s chroma %dx%d %d-bit ctb %d map=%s sl=%s borders=%s variant=%#x fused=%d in_place=%d" % (
        kind, {1: "2:0", 2: "2:2", 3: "4:4"}[cf], w, h, bd, 1 << ctb_y, qmap is not None, so is not None, bo is not None, variant, fused, in_place)
    return what, bad, edge, pad_diff


def _fmt(cf):
    return {1: "420", 2: "422", 3: "444"}[cf]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0, help="stop after this long (0 = run all cases)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    t0, done, mism, first, edge, pad_diff = time.time(), 0, 0, None, 0, 0
    kinds = {}
    for _ in range(a.cases):
        what, bad, e, pd = one_case(ctx, rng)
        done += 1
        edge += e
        pad_diff += pd
        kinds[what.split()[0]] = kinds.get(what.split()[0], 0) + 1
        if bad:
            mism += 1
            first = first or what
        if a.seconds and time.time() - t0 > a.seconds:
            break
    print(json.dumps({"soak": "g4", "seed": a.seed, "cases": done, "by_entry": kinds, "mismatching_cases": mism, "first_mismatch": first,
                      "samples_changed_at_the_new_last_edges": edge, "samples_padding_would_get_wrong": pad_diff,
                      "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
