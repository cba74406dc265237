#!/usr/bin/env python3
"""Random soak of the _sp entry (a semi-planar chroma plane: interleaved Cb / Cr pairs, both components deblocked in one launch)
against tests/sp_ref.py: each case draws a plane size (multiples of 4 per component), a bit depth of 8 .. 14, one QP or a QP map, the
two cQpPicOffsets and a tc offset, bS arrays with keep flags, per-slice pairs or none, a row pitch on either side of the packed
kernels' guard, a kernel variant (32-bit / packed / automatic) and in place or not -- runs it on device 0 through the Python package (DeviceBatch(semi_planar=True)) and compares every byte, row padding included.
Prints one JSON line; exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
import g4_ref as G  # noqa: E402
import slice_offsets_ref as R  # noqa: E402
import sp_ref as S  # noqa: E402

FILL = 0x5A


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    if a.nbytes:
        d.upload(a.view(np.uint8).ravel())
    return d


def one_case(ctx, rng):
    """-> (description, mismatching bytes, samples changed per component)"""
    bd = int(rng.choice([8, 9, 10, 12, 13, 14]))
    sb = 1 if bd == 8 else 2
    w, h = 4 * int(rng.integers(2, 90)), 4 * int(rng.integers(2, 40))
    word = 4 * sb   # one 4-sample word: what every kernel needs; half a block's row (2 words) is what the packed kernels need
    pitch = 2 * w * sb + word * int(rng.integers(0, 5))
    in_place = bool(rng.integers(0, 2))
    frame = S.merge(*[G.blocky_plane(w, h, bd, rng) if rng.integers(0, 4) else G.noise_plane(w, h, bd, rng) for _ in range(2)])
    b = deblock.DeviceBatch(ctx, w, h, 1, bit_depth=bd, per_frame_bs=False, pitch=pitch, in_place=in_place, semi_planar=True)
    b.upload_all(frame[None], fill=FILL)
    if not in_place:
        b.dst.upload(np.full(b.frame_bytes // b.sb, FILL, b.dtype))
    free = []
    vb, hb = G.random_bs(w, h, rng)
    b.set_bs(0, vb, hb)
    u = int(rng.choice([3, 4, 6]))
    qmap = rng.integers(18, 52, (-(-2 * h >> u), -(-2 * w >> u))).astype(np.uint8) if rng.integers(0, 2) else None
    if qmap is not None:
        b.set_qp_map(qmap, u)
    qp = int(rng.integers(18, 52))
    hp = dict(tc_offset_div2=int(rng.integers(-6, 7)), cb_qp_offset=int(rng.integers(-12, 13)), cr_qp_offset=int(rng.integers(-12, 13)))
    so = pairs = None
    ctb_y = int(rng.choice([4, 5, 6]))
    if rng.integers(0, 2):
        rows, cols = -(-2 * h >> ctb_y), -(-2 * w >> ctb_y)
        sidx = R.slices_raster(rows, cols, int(rng.integers(1, rows * cols + 1)))
        pairs = R.ctb_pairs(sidx, rng.integers(-6, 7, (int(sidx.max()) + 1, 2)).astype(np.int8))
        dso = up(ctx, pairs)
        free.append(dso)
        so = _lib.SliceOffsets(dso.ptr, cols, 0, ctb_y)
    variant = int(rng.choice([_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED, _lib.KERNEL_PACKED | _lib.MAP_ROWS]))
    want = S.deblock(frame, vb, hb, qp=qp, qp_map=qmap, unit_log2=u, bit_depth=bd, slice_pairs=pairs, sl_ctb_log2=ctb_y, **hp)
    try:
        ctx.filter_device_h265(b.planes(), qp, variant=variant, slice_offsets=so, semi_planar=True, **hp)
    except deblock.DeblockError as e:   # depth or pitch the packed kernels do not take
        if e.code != _lib.ERR_UNSUPPORTED or (variant & 0xff) != _lib.KERNEL_PACKED:
            raise
        ctx.filter_device_h265(b.planes(), qp, variant=_lib.KERNEL_AUTO, slice_offsets=so, semi_planar=True, **hp)
    what = "dbk %dx%d %d-bit pitch+%d map=%s sl=%s variant=%#x in_place=%d" % (w, h, bd, pitch - 2 * w * sb, qmap is not None,
                                                                             so is not None, variant, in_place)
    ctx.synchronize()
    got = b.download_frame(0, with_padding=True)
    bad = int((got[:, : 2 * w].reshape(h, w, 2) != want).sum())
    bad += int((got[:, 2 * w:] != FILL).sum())   # the row padding
    changed = [int((want[..., k] != frame[..., k]).sum()) for k in range(2)]
    if b.qp_map is not None:
        b.qp_map.free()
    b.free()
    for x in free:
        x.free()
    return what, bad, changed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0, help="stop after this long (0 = run all cases)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    t0, done, mism, first, changed = time.time(), 0, 0, None, [0, 0]
    kinds = {}
    for _ in range(a.cases):
        what, bad, ch = one_case(ctx, rng)
        done += 1
        changed = [changed[k] + ch[k] for k in range(2)]
        key = what.split("variant=")[1].split()[0]
        kinds[key] = kinds.get(key, 0) + 1
        if bad:
            mism += 1
            first = first or what
        if a.seconds and time.time() - t0 > a.seconds:
            break
    print(json.dumps({"soak": "sp", "seed": a.seed, "cases": done, "by_variant": kinds, "mismatching_cases": mism, "first_mismatch": first,
                      "samples_changed_per_component": changed, "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
