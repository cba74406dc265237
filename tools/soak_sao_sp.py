#!/usr/bin/env python3
"""Random soak of hevcdbk_sao_filter_device_sp (SAO of a semi-planar chroma plane: interleaved Cb / Cr pairs, both components in one
launch, each with its own CTB parameters) against tests/sao_sp_ref.py: each case draws a plane size (multiples of 4 per component), a
bit depth of 8 .. 14, square CTBs of 8 / 16 / 32, the two components' parameters -- agreeing in type and class in most CTBs, as a
stream has them, and disagreeing in the rest -- a keep map or none, a slice / tile layout or none and a row pitch on either side of the
packed kernels' guard, runs it on device 0 through the Python package (DeviceBatch(semi_planar=True)) and compares every byte, row
padding included.  Prints one JSON line; exit status 1 on a mismatch."""
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
import sp_ref as S  # noqa: E402

FILL = 0x5A


def up(ctx, a):
    a = np.ascontiguousarray(a)
    d = ctx.alloc(max(a.nbytes, 1))
    if a.nbytes:
        d.upload(a.view(np.uint8).ravel())
    return d


def one_case(ctx, rng):
    """-> (description, mismatching bytes, samples changed per component, CTBs agreeing, CTBs)"""
    bd = int(rng.choice([8, 9, 10, 12, 13, 14]))
    sb = 1 if bd == 8 else 2
    w, h = 4 * int(rng.integers(2, 90)), 4 * int(rng.integers(2, 40))
    lg = int(rng.choice([3, 4, 5]))
    word = 4 * sb   # one 4-sample word: what every kernel needs; a lane's row piece (4 words) is what the packed kernels need
    pitch = 2 * w * sb + word * int(rng.integers(0, 9))
    if rng.integers(0, 2):   # half of the cases on the packed side of the pitch guard
        pitch = -(-pitch // (4 * word)) * (4 * word)
    frame = S.merge(*[G.noise_plane(w, h, bd, rng) if rng.integers(0, 4) else G.blocky_plane(w, h, bd, rng) for _ in range(2)])
    b = deblock.DeviceBatch(ctx, w, h, 1, bit_depth=bd, per_frame_bs=False, pitch=pitch, semi_planar=True)
    b.upload_all(frame[None], fill=FILL)
    b.dst.upload(np.full(b.frame_bytes // b.sb, FILL, b.dtype))
    pcb, pcr = rx.random_sao_params(w, h, lg, lg, rng, bd), rx.random_sao_params(w, h, lg, lg, rng, bd)
    agree = rng.random(pcb.shape) < 0.7
    pcr["type"] = np.where(agree, pcb["type"], pcr["type"])
    pcr["cls"] = np.where(agree & (pcb["type"] == 2), pcb["cls"], pcr["cls"])
    rows, cols = pcb.shape
    keep = G.keep_map(w, h, rng, p=0.2) if rng.integers(0, 2) else None
    layout = B._layout_of(str(rng.choice(["tiles", "slices", "mixed", "random"])), rows, cols, rng) if rng.integers(0, 2) else None
    free = [up(ctx, pcb), up(ctx, pcr)]
    kw = {}
    if keep is not None:
        free.append(up(ctx, keep))
        kw.update(keep_ptr=free[-1].ptr, keep_stride=keep.shape[1])
    if layout is not None:
        nox = np.ascontiguousarray(B.expected_nox(layout), np.uint8)
        free.append(up(ctx, nox))
        kw.update(borders=_lib.SaoBorders(free[-1].ptr, nox.shape[1], 0))
    assert b.keep_shape == ((h + 7) // 8, (w + 7) // 8) and b.ctb_shape(lg) == (rows, cols)
    want = P.sao(frame, pcb, pcr, lg, bd, keep=keep, layout=layout)
    ctx.sao_device(b.planes(), free[0].ptr, cols, lg, semi_planar=True, params_cr_ptr=free[1].ptr, **kw)
    packed = bd <= 12 and pitch % (16 * sb) == 0
    what = "sao %dx%d %d-bit ctb=%d pitch+%d keep=%s layout=%s kernel=%s" % (w, h, bd, 1 << lg, pitch - 2 * w * sb, keep is not None,
                                                                            layout is not None, "packed" if packed else "per-sample")
    ctx.synchronize()
    got = b.download_frame(0, with_padding=True)
    bad = int((got[:, : 2 * w].reshape(h, w, 2) != want).sum())
    bad += int((got[:, 2 * w:] != FILL).sum())   # the row padding
    changed = [int((want[..., k] != frame[..., k]).sum()) for k in range(2)]
    same = (pcb["type"] == pcr["type"]) & ((pcb["type"] != 2) | (pcb["cls"] == pcr["cls"]))
    b.free()
    for x in free:
        x.free()
    return what, bad, changed, int(same.sum()), int(same.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=3000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0, help="stop after this long (0 = run all cases)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    ctx = deblock.Context(0)
    t0, done, mism, first, changed, agree, ctbs = time.time(), 0, 0, None, [0, 0], 0, 0
    kinds = {}
    for _ in range(a.cases):
        what, bad, ch, ag, n = one_case(ctx, rng)
        done += 1
        changed = [changed[k] + ch[k] for k in range(2)]
        agree, ctbs = agree + ag, ctbs + n
        key = what.split("kernel=")[1]
        kinds[key] = kinds.get(key, 0) + 1
        if bad:
            mism += 1
            first = first or what
        if a.seconds and time.time() - t0 > a.seconds:
            break
    print(json.dumps({"soak": "sao_sp", "seed": a.seed, "cases": done, "by_kernel": kinds, "mismatching_cases": mism, "first_mismatch": first,
                      "samples_changed_per_component": changed, "ctbs_agreeing": agree, "ctbs": ctbs, "seconds": round(time.time() - t0, 1)}))
    ctx.close()
    return 1 if mism else 0


if __name__ == "__main__":
    sys.exit(main())
