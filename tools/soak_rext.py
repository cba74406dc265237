#!/usr/bin/env python3
"""Random soak of the chroma formats of the spec-exact mode against the oracles: each case draws a chroma format (4:0:0,
4:2:0, 4:2:2, 4:4:4), a picture size, a bit depth, one QP or a QP map (unit 8..64), bS arrays, tc / beta / cb / cr offsets,
SAO parameters (CtbSizeY 16..64) and an entry point -- deblocking + SAO of Y, Cb, Cr in one call with fused AUTO / ON / OFF,
or the deblocking filter alone on one plane with kernel AUTO / GENERIC / PACKED -- runs it on device 0 and compares every
byte with oracle/h265.py (luma) and tests/rext_oracle.py (chroma, SAO).  Prints one JSON line; exit status 1 on a mismatch."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_video_codec_amd import deblock, _lib  # noqa: E402
from oracle import h265  # noqa: E402
import rext_oracle as rx  # noqa: E402

FMTS = {"400": 0, "420": 1, "422": 2, "444": 3}


def blocky(rng, w, h, bd):
    top = (1 << bd) - 1
    base = rng.integers(top // 4, 3 * top // 4, (h // 8 + 1, w // 8 + 1))
    p = np.kron(base, np.ones((8, 8), np.int64))[:h, :w] + rng.integers(-3, 4, (h, w)) * (1 << (bd - 8))
    if rng.integers(0, 2):
        p[: h // 4, : w // 4] = rng.integers(0, top + 1, (h // 4, w // 4))
    return np.clip(p, 0, top).astype(np.uint8 if bd == 8 else np.uint16)


def rand_bs(rng, w, h):
    mk = lambda n: rng.integers(0, 3, n) | (rng.integers(0, 10, n) == 0) * rx.KEEP_P | (rng.integers(0, 10, n) == 0) * rx.KEEP_Q
    return mk((w // 8 + 1) * (h // 4)).astype(np.uint8), mk((h // 8 + 1) * (w // 4)).astype(np.uint8)


def one_case(ctx, rng):
    fmt = str(rng.choice(list(FMTS)))
    cf = FMTS[fmt]
    sx, sy = rx.SUB.get(cf, (1, 1))
    bd = int(rng.choice([8, 10, 12]))
    # luma sizes whose chroma planes are multiples of 8 (4:2:0 also in both axes: its own entry's rule)
    w = 16 * int(rng.integers(1, 17))
    h = (16 if cf == 1 else 8) * int(rng.integers(1, 17))
    n = int(rng.integers(1, 3))
    qp = int(rng.integers(15, 52))
    unit_log2 = int(rng.integers(3, 7))
    qmap = rng.integers(15, 52, (-(-h >> unit_log2), -(-w >> unit_log2))).astype(np.uint8) if rng.integers(0, 2) else None
    prm = dict(tc_offset_div2=int(rng.integers(-6, 7)), beta_offset_div2=int(rng.integers(-6, 7)),
               cb_qp_offset=int(rng.integers(-12, 13)), cr_qp_offset=int(rng.integers(-12, 13)))
    vb, hb = rand_bs(rng, w, h)
    nplanes = 1 if cf == 0 else 3
    geo = [(w, h)] + [(w // sx, h // sy)] * (nplanes - 1)
    bss = [(vb, hb)] + ([rx.chroma_bs(vb, hb, w, h, cf)] * 2 if cf else [])
    frames = [np.stack([blocky(rng, pw, ph, bd) for _ in range(n)]) for pw, ph in geo]
    keep = []

    def dbk_want(i, f):
        if i == 0:
            return h265.filter_plane(frames[0][f], qp, vb, hb, bit_depth=bd, qp_map=qmap, unit_log2=unit_log2,
                                     tc_offset_div2=prm["tc_offset_div2"], beta_offset_div2=prm["beta_offset_div2"])
        return rx.filter_chroma_plane(frames[i][f], bss[i][0], bss[i][1], cf, qp=qp, qp_map=qmap, unit_log2=unit_log2, bit_depth=bd,
                                      tc_offset_div2=prm["tc_offset_div2"],
                                      c_qp_offset=prm["cb_qp_offset"] if i == 1 else prm["cr_qp_offset"])

    def planes_of(i):
        b = deblock.DeviceBatch(ctx, geo[i][0], geo[i][1], n, bit_depth=bd, is_chroma=i > 0, per_frame_bs=False)
        b.upload_all(frames[i])
        dv, dh = ctx.alloc(bss[i][0].size), ctx.alloc(bss[i][1].size)
        dv.upload(bss[i][0])
        dh.upload(bss[i][1])
        if qmap is not None:
            b.set_qp_map(qmap, unit_log2)
            keep.append(b.qp_map)
        keep.extend([b, dv, dh])
        p = b.planes()
        p.vert_bs, p.hor_bs, p.vert_bs_stride, p.hor_bs_stride = dv.ptr, dh.ptr, 0, 0
        return b, p

    desc = {"fmt": fmt, "w": w, "h": h, "n": n, "bd": bd, "qp": qp, "map": None if qmap is None else unit_log2, **prm}
    try:
        if rng.integers(0, 4) == 0:  # the deblocking filter alone, one plane
            i = int(rng.integers(0, nplanes))
            variant = int(rng.choice([_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_PACKED]))
            desc.update(entry="filter", plane=i, variant=variant)
            b, p = planes_of(i)
            try:
                ctx.filter_device_h265(p, qp, c_idx=i, variant=variant, chroma_format=fmt, **prm)
            except deblock.DeblockError as e:
                if e.code == _lib.ERR_UNSUPPORTED and variant == _lib.KERNEL_PACKED:
                    return desc, "unsupported", True
                raise
            ctx.synchronize()
            ok = all(np.array_equal(b.download_frame(f), dbk_want(i, f)) for f in range(n))
            return desc, "ran", ok
        ctb_y = int(rng.choice([4, 5, 6]))
        fused = int(rng.choice([_lib.FUSED_AUTO, _lib.FUSED_ON, _lib.FUSED_OFF]))
        desc.update(entry="deblock_sao_planes", ctb_y=ctb_y, fused=fused)
        sao, want, bs_ = [], [], []
        for i in range(nplanes):
            lw, lh = (ctb_y, ctb_y) if i == 0 else (ctb_y - (sx - 1), ctb_y - (sy - 1))
            p_ = np.stack([rx.random_sao_params(geo[i][0], geo[i][1], lw, lh, rng, bd) for _ in range(n)])
            dp = ctx.alloc(p_.nbytes)
            dp.upload(np.ascontiguousarray(p_).view(np.uint8))
            keep.append(dp)
            sao.append({"params": dp.ptr, "params_stride": p_.shape[2], "ctb_log2": lw, "params_frame_stride": p_.shape[1] * p_.shape[2]})
            want.append([rx.sao_plane(dbk_want(i, f), p_[f], lw, lh, bit_depth=bd) for f in range(n)])
            bs_.append(planes_of(i))
        try:
            ctx.deblock_sao_device_planes([p for _, p in bs_], qp, sao, h265=prm, fused=fused, chroma_format=fmt)
        except deblock.DeblockError as e:
            if e.code == _lib.ERR_UNSUPPORTED and fused == _lib.FUSED_ON:
                return desc, "unsupported", True
            raise
        ctx.synchronize()
        ok = all(np.array_equal(bs_[i][0].download_frame(f), want[i][f]) for i in range(nplanes) for f in range(n))
        return desc, "ran", ok
    finally:
        for x in keep:
            x.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    counts, bad, t0 = {}, [], time.time()
    for k in range(a.cases):
        desc, what, ok = one_case(ctx, rng)
        key = "%s/%s/%s" % (desc["fmt"], desc["entry"], what)
        counts[key] = counts.get(key, 0) + 1
        if not ok:
            bad.append(dict(desc, case=k))
    ctx.close()
    print(json.dumps({"soak": "chroma formats, spec-exact deblocking + SAO", "seed": a.seed, "cases": a.cases,
                      "mismatches": len(bad), "first_mismatches": bad[:5], "counts": dict(sorted(counts.items())),
                      "wall_s": round(time.time() - t0, 1)}))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
