"""The --borders layouts of tools/bench_sao.py and tools/bench_deblock_sao.py: per-CTB slice / tile arrays for
Context.derive_sao_borders, and the share of 64 x 64 regions (the SAO waves of a picture with 64-sample CTBs) that take the
masked form -- a region does when one of its blocks has a direction not to look in: its CTB's byte is not zero, or it lies on
the picture border (those take the border form without the operand as well)."""
import numpy as np

KINDS = ["none", "zero", "decoder", "every-ctb"]


def arrays(kind, rows, cols):
    """(slice_idx, slice_across, tile_idx, tiles_across) per CTB; `zero`: one slice, one tile -- nothing forbidden"""
    yy, xx = np.mgrid[0:rows, 0:cols]
    if kind == "zero":
        z = np.zeros((rows, cols), np.uint16)
        return z, np.ones((rows, cols), np.uint8), z, True
    if kind == "decoder":     # 2 x 2 tiles not to be crossed; in every tile a slice every 8 CTB rows, flag 0
        ty, tx = (yy >= rows // 2).astype(np.int64), (xx >= cols // 2).astype(np.int64)
        tile = ty * 2 + tx
        per_tile = rows // 8 + 2
        sl = tile * per_tile + (yy - ty * (rows // 2)) // 8   # rises with the decoding (tile-scan) order
        return sl.astype(np.uint16), np.zeros((rows, cols), np.uint8), tile.astype(np.uint16), False
    if kind == "every-ctb":   # each CTB a slice of its own, flag 0: every CTB border forbidden
        return (yy * cols + xx).astype(np.uint16), np.zeros((rows, cols), np.uint8), np.zeros((rows, cols), np.uint16), True
    raise ValueError(kind)


def device_borders(ctx, kind, rows, cols):
    """(_lib.SaoBorders or None, device buffer or None, share of masked regions) for one picture, shared by a batch"""
    from gpu_video_codec_amd import _lib
    if kind == "none":
        return None, None, None
    s, a, t, across = arrays(kind, rows, cols)
    nox = np.ascontiguousarray(ctx.derive_sao_borders(s, a, t, tiles_across=across))
    rim = np.zeros((rows, cols), bool)
    rim[0] = rim[-1] = rim[:, 0] = rim[:, -1] = True
    buf = ctx.alloc(nox.nbytes)
    buf.upload(nox)
    return _lib.SaoBorders(buf.ptr, cols, 0), buf, float(((nox != 0) | rim).mean())
