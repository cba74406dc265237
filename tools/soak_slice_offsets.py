#!/usr/bin/env python3
"""Random soak of the per-slice deblocking offsets (H.265 8.7.2.5.3 / 8.7.2.5.5) against the composition of
tests/slice_offsets_ref.py: each case draws a chroma format, a picture size, a bit depth, a CTB size, a slice layout (raster runs or
bands of CTB rows), a table of pairs, one QP or a QP map, bS arrays with keep flags, the pairs from the producer
hevcdbk_h265_slice_offsets_device, and an entry -- deblocking only (32-bit / packed / automatic kernel, in place or not) on every
plane, or deblocking + SAO of the picture's planes in one call with fused AUTO / ON / OFF -- runs it on device 0 and compares every
byte.  Prints one JSON line; exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
import rext_oracle as rx  # noqa: E402
import slice_offsets_ref as R  # noqa: E402
from soak_sao_borders import FMTS, rand_bs, up  # noqa: E402


def one_case(ctx, rng):
    """-> (description, mismatching bytes, bytes that differ from the zero-offset result)"""
    fmt = str(rng.choice(list(FMTS)))
    cf = FMTS[fmt]
    sx, sy = rx.SUB.get(cf, (1, 1))
    bd = int(rng.choice([8, 10, 12]))
    sb = 1 if bd == 8 else 2
    w = 16 * int(rng.integers(1, 21))
    h = (16 if cf == 1 else 8) * int(rng.integers(1, 21))
    ctb_y = int(rng.choice([4, 5, 6]))
    rows, cols = -(-h >> ctb_y), -(-w >> ctb_y)
    if rng.integers(0, 2):
        sidx = R.slices_raster(rows, cols, int(rng.integers(1, rows * cols + 1)))
    else:
        sidx = R.slices_every_rows(rows, cols, int(rng.integers(1, rows + 1)))
    n_slices = int(sidx.max()) + 1
    table = rng.integers(-6, 7, (n_slices, 2)).astype(np.int8)
    n_used = n_slices if rng.integers(0, 4) else max(n_slices // 2, 1)   # now and then a table that is too short: (0, 0)
    pairs = ctx.derive_slice_offsets(sidx, table[:n_used])
    bad = int((pairs != R.ctb_pairs(sidx, table[:n_used])).sum())
    dso = up(ctx, pairs)
    so = _lib.SliceOffsets(dso.ptr, cols, 0, ctb_y)
    use_map = bool(rng.integers(0, 2))
    u = int(rng.choice([3, 4, 6]))
    qmap = rng.integers(18, 52, (-(-h >> u), -(-w >> u))).astype(np.uint8) if use_map else None
    qp = int(rng.integers(18, 52))
    vb, hb = rand_bs(rng, w, h)
    with_sao = bool(rng.integers(0, 2))
    fused = int(rng.choice([_lib.FUSED_AUTO, _lib.FUSED_ON, _lib.FUSED_OFF]))
    variant = int(rng.choice([_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED]))
    in_place = bool(rng.integers(0, 2)) and not with_sao
    hp = dict(tc_offset_div2=int(rng.integers(-6, 7)), beta_offset_div2=int(rng.integers(-6, 7)), cb_qp_offset=int(rng.integers(-4, 5)),
              cr_qp_offset=int(rng.integers(-4, 5)))   # the two offsets must not matter
    free, batches, planes, sao, want = [dso], [], [], [], []
    bite = 0
    for i in range(1 if cf == 0 else 3):
        pw, ph = (w, h) if i == 0 else (w // sx, h // sy)
        lw, lh = (ctb_y, ctb_y) if i == 0 else (ctb_y - (sx - 1), ctb_y - (sy - 1))
        frame = rng.integers(0, 1 << bd, (ph, pw)).astype(np.uint8 if sb == 1 else np.uint16)
        frame[: ph // 2] = (frame[: ph // 2] >> 4) + (1 << (bd - 2))
        b_v, b_h = (vb, hb) if i == 0 else rx.chroma_bs(vb, hb, w, h, cf)
        b = deblock.DeviceBatch(ctx, pw, ph, 1, bit_depth=bd, is_chroma=i > 0, per_frame_bs=False, in_place=in_place)
        b.upload_all(frame[None])
        dv, dh = up(ctx, b_v), up(ctx, b_h)
        free += [dv, dh]
        if qmap is not None:
            b.set_qp_map(qmap, u)
        p = b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
        batches.append(b)
        planes.append(p)
        kw = dict(qp=qp, c_idx=i, chroma_format=max(cf, 1), qp_map=qmap, unit_log2=u, bit_depth=bd,
                  c_qp_offset=0 if i == 0 else (hp["cb_qp_offset"] if i == 1 else hp["cr_qp_offset"]))
        d = R.expected(frame, b_v, b_h, pairs, ctb_y, **kw)
        zero = R.expected(frame, b_v, b_h, np.zeros_like(pairs), ctb_y, **kw)
        bite += int((d != zero).sum())
        if with_sao:
            prm = rx.random_sao_params(pw, ph, lw, lh, rng, bd)
            dp = up(ctx, prm)
            free.append(dp)
            sao.append({"params": dp.ptr, "params_stride": prm.shape[1], "ctb_log2": lw, "ctb_log2_h": lh})
            d = rx.sao_plane(d, prm, lw, lh, bit_depth=bd)
        want.append(d)
    if with_sao:
        try:
            ctx.deblock_sao_device_planes(planes, qp, sao, h265=hp, fused=fused, chroma_format=fmt, slice_offsets=so)
        except deblock.DeblockError as e:   # operands the fused kernel does not take with or without the operand
            if e.code != _lib.ERR_UNSUPPORTED or fused != _lib.FUSED_ON:
                raise
            ctx.deblock_sao_device_planes(planes, qp, sao, h265=hp, fused=_lib.FUSED_AUTO, chroma_format=fmt, slice_offsets=so)
    else:
        for i, p in enumerate(planes):
            kw = dict(c_idx=i, chroma_format=fmt, slice_offsets=so, **hp)
            try:
                ctx.filter_device_h265(p, qp, variant=variant, **kw)
            except deblock.DeblockError as e:   # no packed kernel for this plane, with or without the operand
                if e.code != _lib.ERR_UNSUPPORTED or variant != _lib.KERNEL_PACKED:
                    raise
                ctx.filter_device_h265(p, qp, variant=_lib.KERNEL_AUTO, **kw)
    ctx.synchronize()
    for i, b in enumerate(batches):
        bad += int((b.download_frame(0) != want[i]).sum())
        if b.qp_map is not None:
            b.qp_map.free()
        b.free()
    for x in free:
        x.free()
    return "%s %dx%d %d-bit ctb %d slices %d map=%s %s" % (fmt, w, h, bd, 1 << ctb_y, n_slices, use_map,
                                                           "dbk+sao fused=%d" % fused if with_sao else "dbk variant=%d in_place=%d" % (variant, in_place)), bad, bite


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0, help="stop after this long (0 = run all cases)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    t0, done, mism, bite, biting, first = time.time(), 0, 0, 0, 0, None
    for _ in range(a.cases):
        what, bad, b = one_case(ctx, rng)
        done += 1
        bite += b
        biting += b > 0
        if bad:
            mism += 1
            first = first or what
        if a.seconds and time.time() - t0 > a.seconds:
            break
    print(json.dumps({"soak": "slice_offsets", "seed": a.seed, "cases": done, "mismatching_cases": mism, "first_mismatch": first,
                      "cases_differing_from_zero_offsets": biting, "bytes_differing_from_zero_offsets": bite, "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
