"""Per-slice deblocking offsets (H.265 8.7.2.5.3 luma, 8.7.2.5.5 chroma): the expected picture, built from the existing checkers
alone -- oracle/h265.py::filter_plane (luma, 4:2:0 chroma) and tests/rext_oracle.py::filter_chroma_plane (4:2:2 / 4:4:4 chroma),
both of which take ONE pair of offsets per call.

8.7.2 filters every 8-grid edge segment of a direction independently of the others, and its result depends only on that segment's
parameters.  So the picture with per-slice offsets is a composition of uniform-offset runs:
  vertical pass    for each distinct pair, one run with that pair as uniform offsets and the horizontal bS zeroed; sample (x, y)
                   takes the run of the pair owned by the CTB at luma (((x + 4) // 8) * 8 * SubWidthC, y * SubHeightC) -- the CTB
                   that holds q0 of the vertical edge the sample belongs to;
  horizontal pass  the same on the composed picture with the vertical bS zeroed and the selector ((y + 4) // 8) * 8.
selector="p" composes with the CTB on the P side of the edge instead -- the one-character mistake the feature invites -- for the
census of test_slice_offsets_cpu.py.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED like the rest of the spec-exact mode."""
import numpy as np

import rext_oracle as rx

PAIRS = [(-6, -6), (6, 6), (0, -3), (3, 0), (-2, 5)]   # (slice_beta_offset_div2, slice_tc_offset_div2)


def slices_raster(rows, cols, run, first=0):
    """slice index per CTB: slices of `run` CTBs in raster order"""
    return ((np.arange(rows * cols) // run) + first).reshape(rows, cols).astype(np.uint16)


def slices_every_rows(rows, cols, k):
    """a slice every k CTB rows"""
    return np.repeat((np.arange(rows) // k)[:, None], cols, 1).astype(np.uint16)


def table_for(n_slices, pairs=PAIRS, shift=0):
    """the slice table (n_slices, 2): the pairs in turn"""
    return np.array([pairs[(i + shift) % len(pairs)] for i in range(n_slices)], np.int8).reshape(n_slices, 2)


def ctb_pairs(slice_idx, table):
    """what the producer writes: (rows, cols, 2) int8, (0, 0) for a slice index the table does not hold"""
    si = np.asarray(slice_idx, np.int64)
    tb = np.asarray(table, np.int8).reshape(-1, 2)
    out = np.zeros(si.shape + (2,), np.int8)
    ok = si < tb.shape[0]
    out[ok] = tb[si[ok]]
    return out


def ctb_pairs_per_sample(slice_of_sample, table, ctb_log2):
    """the same bytes gathered from per-sample slice membership ((H, W) array of slice indices): the CTB's top-left sample"""
    s = np.asarray(slice_of_sample)
    return ctb_pairs(s[:: 1 << ctb_log2, :: 1 << ctb_log2], table)


def _run(plane, vb, hb, pair, c_idx, cf, kw):
    from oracle import h265
    beta, tc = int(pair[0]), int(pair[1])
    if c_idx == 0 or cf == 1:
        return h265.filter_plane(plane, kw["qp"], vb, hb, c_idx=c_idx, bit_depth=kw["bit_depth"], qp_map=kw["qp_map"],
                                 unit_log2=kw["unit_log2"], tc_offset_div2=tc, beta_offset_div2=beta, c_qp_offset=kw["c_qp_offset"])
    return rx.filter_chroma_plane(plane, vb, hb, cf, qp=kw["qp"], qp_map=kw["qp_map"], unit_log2=kw["unit_log2"],
                                  bit_depth=kw["bit_depth"], c_qp_offset=kw["c_qp_offset"], tc_offset_div2=tc)


def expected(plane, vert_bs4, hor_bs4, pairs, ctb_log2, *, qp, c_idx=0, chroma_format=1, qp_map=None, unit_log2=3, bit_depth=8,
             c_qp_offset=0, selector="q"):
    """the deblocked plane under per-CTB pairs (rows, cols, 2) of the LUMA CTB grid; plane = luma (c_idx 0) or a chroma plane of a
    picture in chroma_format 1..3"""
    plane = np.ascontiguousarray(plane)
    h, w = plane.shape
    sx, sy = (1, 1) if c_idx == 0 else rx.SUB[chroma_format]
    lw, lh = w * sx, h * sy
    pairs = np.asarray(pairs, np.int8)
    vb = np.ascontiguousarray(vert_bs4, np.uint8)
    hb = np.ascontiguousarray(hor_bs4, np.uint8)
    kw = dict(qp=qp, qp_map=qp_map, unit_log2=unit_log2, bit_depth=bit_depth, c_qp_offset=c_qp_offset)
    side = 0 if selector == "q" else -1   # "p": the last sample before the edge
    yy, xx = np.mgrid[0:h, 0:w]

    def owner(ex, ey):
        """pair index array: the CTB at luma (ex * sx, ey * sy), clamped into the picture"""
        cx = np.clip(ex * sx, 0, lw - 1) >> ctb_log2
        cy = np.clip(ey * sy, 0, lh - 1) >> ctb_log2
        return pairs[cy, cx]

    def compose(src, v, hh, own):
        out = src.copy()
        for pr in np.unique(own.reshape(-1, 2), axis=0):
            run = _run(src, v, hh, pr, c_idx, chroma_format, kw)
            m = (own[..., 0] == pr[0]) & (own[..., 1] == pr[1])
            out[m] = run[m]
        return out

    ver = compose(plane, vb, np.zeros_like(hb), owner(((xx + 4) // 8) * 8 + side, yy))
    return compose(ver, np.zeros_like(vb), hb, owner(xx, ((yy + 4) // 8) * 8 + side))


def cells_differ(a, b, cell=32):
    """True when a and b differ somewhere in EVERY cell x cell block of the plane"""
    d = np.asarray(a) != np.asarray(b)
    h, w = d.shape
    d = d[: h - h % cell, : w - w % cell]
    return bool(d.reshape(h // cell, cell, w // cell, cell).any(axis=(1, 3)).all())
