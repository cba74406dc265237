#!/usr/bin/env python3
"""Random soak of SAO and deblocking + SAO at slice / tile boundaries not to be crossed (H.265 8.7.3.2) against the per-sample
statement of tests/sao_borders_ref.py: each case draws a chroma format, a picture size, a bit depth, a CTB size, one QP or a QP
map, bS arrays, edge-heavy SAO parameters, a layout of tiles and slices with drawn flags (or every CTB a slice of its own), the
bytes from the producer hevcdbk_h265_sao_borders_device, and an entry -- the SAO pass on one plane, or deblocking + SAO of the
picture's planes in one call with fused AUTO / ON / OFF -- runs it on device 0 and compares every byte.  Prints one JSON line;
exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
from oracle import h265  # noqa: E402
import rext_oracle as rx  # noqa: E402
import sao_borders_ref as R  # noqa: E402

FMTS = {"400": 0, "420": 1, "422": 2, "444": 3}


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    d.upload(a.view(np.uint8).ravel())
    return d


def rand_bs(rng, w, h):
    mk = lambda n: rng.integers(0, 3, n) | (rng.integers(0, 10, n) == 0) * rx.KEEP_P | (rng.integers(0, 10, n) == 0) * rx.KEEP_Q
    return mk((w // 8 + 1) * (h // 4)).astype(np.uint8), mk((h // 8 + 1) * (w // 4)).astype(np.uint8)


def one_case(ctx, rng):
    """-> (description, mismatching bytes, bytes that differ from the border-less result)"""
    fmt = str(rng.choice(list(FMTS)))
    cf = FMTS[fmt]
    sx, sy = rx.SUB.get(cf, (1, 1))
    bd = int(rng.choice([8, 10, 12]))
    sb = 1 if bd == 8 else 2
    w = 16 * int(rng.integers(1, 21))
    h = (16 if cf == 1 else 8) * int(rng.integers(1, 21))
    ctb_y = int(rng.choice([4, 5, 6]))
    rows, cols = -(-h >> ctb_y), -(-w >> ctb_y)
    kind = str(rng.choice(["tiles", "slices", "mixed", "random", "random", "every", "none"]))
    lay = R._layout_of(kind, rows, cols, rng)
    s, a, t = R.per_ctb(lay)
    nox = ctx.derive_sao_borders(s, a, t if rng.integers(0, 4) or not lay["tiles_across"] else None, tiles_across=lay["tiles_across"])
    bad = int((nox != R.expected_nox(lay)).sum())
    dn = up(ctx, nox)
    borders = _lib.SaoBorders(dn.ptr, cols, 0)
    use_map = bool(rng.integers(0, 3) == 0)
    u = int(rng.choice([3, 4, 6]))
    qmap = rng.integers(20, 52, (-(-h >> u), -(-w >> u))).astype(np.uint8) if use_map else None
    qp = int(rng.integers(22, 52))
    vb, hb = rand_bs(rng, w, h)
    sao_only = bool(rng.integers(0, 3) == 0)
    fused = int(rng.choice([_lib.FUSED_AUTO, _lib.FUSED_ON, _lib.FUSED_OFF]))
    hp = dict(tc_offset_div2=int(rng.integers(-2, 3)), beta_offset_div2=int(rng.integers(-2, 3)), cb_qp_offset=int(rng.integers(-4, 5)),
              cr_qp_offset=int(rng.integers(-4, 5)))
    free, batches, planes, sao, want = [dn], [], [], [], []
    bite = 0
    for i in range(1 if cf == 0 else 3):
        pw, ph = (w, h) if i == 0 else (w // sx, h // sy)
        lw, lh = (ctb_y, ctb_y) if i == 0 else (ctb_y - (sx - 1), ctb_y - (sy - 1))
        frame = rng.integers(0, 1 << bd, (ph, pw)).astype(np.uint8 if sb == 1 else np.uint16)
        frame[: ph // 2] = (frame[: ph // 2] >> 4) + (1 << (bd - 2))
        prm = R.edge_params(rows, cols, rng, bd)
        b_v, b_h = (vb, hb) if i == 0 else rx.chroma_bs(vb, hb, w, h, cf)
        b = deblock.DeviceBatch(ctx, pw, ph, 1, bit_depth=bd, is_chroma=i > 0, per_frame_bs=False)
        b.upload_all(frame[None])
        dv, dh, dp = up(ctx, b_v), up(ctx, b_h), up(ctx, prm)
        free += [dv, dh, dp]
        if qmap is not None:
            b.set_qp_map(qmap, u)
        p = b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
        batches.append(b)
        planes.append(p)
        sao.append({"params": dp.ptr, "params_stride": cols, "ctb_log2": lw, "ctb_log2_h": lh})
        if sao_only:
            d = frame
        elif i == 0:
            d = h265.filter_plane(frame, qp, b_v, b_h, bit_depth=bd, qp_map=qmap, unit_log2=u, tc_offset_div2=hp["tc_offset_div2"],
                                  beta_offset_div2=hp["beta_offset_div2"])
        else:
            d = rx.filter_chroma_plane(frame, b_v, b_h, cf, qp=qp, qp_map=qmap, unit_log2=u, bit_depth=bd, tc_offset_div2=hp["tc_offset_div2"],
                                       c_qp_offset=hp["cb_qp_offset"] if i == 1 else hp["cr_qp_offset"])
        want.append(R.sao_plane(d, prm, lw, lh, lay, bit_depth=bd))
        bite += int((want[-1] != rx.sao_plane(d, prm, lw, lh, bit_depth=bd)).sum())
    if sao_only:
        for i, p in enumerate(planes):
            ctx.sao_device(p, sao[i]["params"], cols, sao[i]["ctb_log2"], ctb_log2_h=sao[i]["ctb_log2_h"], borders=borders)
    else:
        try:
            ctx.deblock_sao_device_planes(planes, qp, sao, h265=hp, fused=fused, chroma_format=fmt, borders=borders)
        except deblock.DeblockError as e:
            if e.code != _lib.ERR_UNSUPPORTED or fused != _lib.FUSED_ON:
                raise
            ctx.deblock_sao_device_planes(planes, qp, sao, h265=hp, fused=_lib.FUSED_AUTO, chroma_format=fmt, borders=borders)
    ctx.synchronize()
    for i, b in enumerate(batches):
        bad += int((b.download_frame(0) != want[i]).sum())
        if b.qp_map is not None:
            b.qp_map.free()
        b.free()
    for x in free:
        x.free()
    return "%s %dx%d %d-bit ctb %d %s %s map=%s fused=%d" % (fmt, w, h, bd, 1 << ctb_y, kind, "sao" if sao_only else "dbk+sao", use_map, fused), bad, bite


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
    print(json.dumps({"soak": "sao_borders", "seed": a.seed, "cases": done, "mismatching_cases": mism, "first_mismatch": first,
                      "cases_differing_from_borderless": biting, "bytes_differing_from_borderless": bite, "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
