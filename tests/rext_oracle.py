"""Chroma of the spec-exact mode for every chroma format: a numpy restatement of ITU-T H.265 clauses 8.7.2.5.5 /
8.7.2.5.8 (chroma deblocking) and 8.7.3 (SAO) for any SubWidthC x SubHeightC.

TEST INFRASTRUCTURE ONLY, and PARITY UNPINNED like the rest of the spec-exact mode: no decoder or conformance stream is
available to pin it.  It is written in the standard's picture order -- every vertical edge of the plane, then every
horizontal edge on the result -- and shares no structure with the kernels' offset-block formulation.  Luma does not
depend on the chroma format and stays with oracle/h265.py.  tests/test_rext_cpu.py ties this file to oracle/h265.py
on the operands where the two must agree (4:2:0, and the other formats where Table 8-10 is the identity).

Conventions (include/hevc_deblock.h): a chroma plane is (H / SubHeightC) x (W / SubWidthC); its bS arrays are
4-sample granular in its own geometry (vert: (cw/8+1) x (ch/4), hor: (ch/8+1) x (cw/4)); bits 1:0 = bS, bit 2 / 3 =
keep the P / Q samples.  QP maps hold QpY per (1 << unit_log2) LUMA samples.
"""
import numpy as np

BS_MASK, KEEP_P, KEEP_Q = 3, 4, 8
SUB = {1: (2, 2), 2: (2, 1), 3: (1, 1)}  # chroma_format_idc -> (SubWidthC, SubHeightC), Table 6-1

# Table 8-12, tC' for Q = 0..53
TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24],
                    np.int64)
assert TC_TABLE.size == 54


def chroma_qp_table_8_10(qpi):
    """QpC as a function of qPi for ChromaArrayType == 1 (Table 8-10)"""
    qpi = np.asarray(qpi, np.int64)
    mid = np.array([29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37], np.int64)  # qPi 30..43
    return np.where(qpi < 30, qpi, np.where(qpi > 43, qpi - 6, mid[np.clip(qpi - 30, 0, 13)]))


def chroma_qp(qpi, chroma_format):
    """8.7.2.5.5: Table 8-10 if ChromaArrayType == 1, otherwise QpC = Min(qPi, 51)"""
    if chroma_format == 1:
        return chroma_qp_table_8_10(qpi)
    return np.minimum(np.asarray(qpi, np.int64), 51)


def chroma_tc(qpl, chroma_format, *, c_qp_offset=0, tc_offset_div2=0, bit_depth=8):
    """tC of a chroma edge with bS 2 whose (QpQ + QpP + 1) >> 1 is qpl: tC' at Clip3(0, 53, QpC + 2 + 2 * tc_offset_div2),
    scaled by (1 << (BitDepthC - 8))"""
    qpc = chroma_qp(np.asarray(qpl, np.int64) + c_qp_offset, chroma_format)
    return TC_TABLE[np.clip(qpc + 2 + 2 * tc_offset_div2, 0, 53)] << (bit_depth - 8)


def chroma_bs(vert_bs4, hor_bs4, w, h, chroma_format):
    """the chroma plane's bS arrays from the luma arrays of a w x h picture: bS[xDk * SubWidthC][yDm * SubHeightC]"""
    sx, sy = SUB[chroma_format]
    cw, ch = w // sx, h // sy
    lv = np.asarray(vert_bs4, np.uint8).reshape(h // 4, w // 8 + 1)
    lh = np.asarray(hor_bs4, np.uint8).reshape(h // 8 + 1, w // 4)
    cv = lv[(np.arange(ch // 4) * 4 * sy) // 4][:, (np.arange(cw // 8 + 1) * 8 * sx) // 8]
    chh = lh[(np.arange(ch // 8 + 1) * 8 * sy) // 8][:, (np.arange(cw // 4) * 4 * sx) // 4]
    return np.ascontiguousarray(cv).ravel(), np.ascontiguousarray(chh).ravel()


def _qp_at(qp, qp_map, unit_log2, lx, ly, lw, lh):
    """QpY of the unit covering luma sample (lx, ly), clamped into the w x h luma picture"""
    if qp_map is None:
        return np.full(np.broadcast(lx, ly).shape, min(int(qp), 51), np.int64)
    m = np.asarray(qp_map, np.int64)
    lx = np.clip(lx, 0, lw - 1) >> unit_log2
    ly = np.clip(ly, 0, lh - 1) >> unit_log2
    return m[ly, lx]


def filter_chroma_plane(plane, vert_bs4, hor_bs4, chroma_format, *, qp=0, qp_map=None, unit_log2=3, bit_depth=8,
                        c_qp_offset=0, tc_offset_div2=0):
    """8.7.2 for one chroma plane (ch x cw) of a picture in chroma_format 1..3; returns a new array"""
    sx, sy = SUB[chroma_format]
    out = np.array(plane, np.int64)
    ch, cw = out.shape
    lw, lh = cw * sx, ch * sy
    max_v = (1 << bit_depth) - 1
    vb = np.asarray(vert_bs4, np.int64).reshape(ch // 4, cw // 8 + 1)
    hb = np.asarray(hor_bs4, np.int64).reshape(ch // 8 + 1, cw // 4)

    def tc_of(qpp, qpq):
        qpl = np.minimum((qpp + qpq + 1) >> 1, 51)
        return chroma_tc(qpl, chroma_format, c_qp_offset=c_qp_offset, tc_offset_div2=tc_offset_div2, bit_depth=bit_depth)

    def edge(p1, p0, q0, q1, entry, tc):
        d = np.clip(((q0 - p0) * 4 + p1 - q1 + 4) >> 3, -tc, tc)
        on = (entry & BS_MASK) == 2
        np0 = np.where(on & ((entry & KEEP_P) == 0), np.clip(p0 + d, 0, max_v), p0)
        nq0 = np.where(on & ((entry & KEEP_Q) == 0), np.clip(q0 - d, 0, max_v), q0)
        return np0, nq0

    # vertical edges x = 8k (0 < x < cw), every line; segment of 4 lines = one bS entry, QP from its first line
    xs = np.arange(8, cw, 8)
    if xs.size:
        y = np.arange(ch)
        ent = vb[y // 4][:, xs // 8]
        y0 = (y // 4) * 4
        qpp = _qp_at(qp, qp_map, unit_log2, (xs[None, :] - 1) * sx, y0[:, None] * sy, lw, lh)
        qpq = _qp_at(qp, qp_map, unit_log2, xs[None, :] * sx, y0[:, None] * sy, lw, lh)
        np0, nq0 = edge(out[:, xs - 2], out[:, xs - 1], out[:, xs], out[:, xs + 1], ent, tc_of(qpp, qpq))
        out[:, xs - 1], out[:, xs] = np0, nq0
    # horizontal edges y = 8k (0 < y < ch) on the result, every column
    ys = np.arange(8, ch, 8)
    if ys.size:
        x = np.arange(cw)
        ent = hb[ys // 8][:, x // 4]
        x0 = (x // 4) * 4
        qpp = _qp_at(qp, qp_map, unit_log2, x0[None, :] * sx, (ys[:, None] - 1) * sy, lw, lh)
        qpq = _qp_at(qp, qp_map, unit_log2, x0[None, :] * sx, ys[:, None] * sy, lw, lh)
        np0, nq0 = edge(out[ys - 2], out[ys - 1], out[ys], out[ys + 1], ent, tc_of(qpp, qpq))
        out[ys - 1], out[ys] = np0, nq0
    return out.astype(np.asarray(plane).dtype)


SAO_CTB_DTYPE = np.dtype([("type", "u1"), ("cls", "u1"), ("offset", "i1", (4,))])


def sao_plane(plane, params, ctb_log2_w, ctb_log2_h, *, bit_depth=8, keep=None):
    """8.7.3 on one plane with CTBs of (1 << ctb_log2_w) x (1 << ctb_log2_h) samples (4:2:2 chroma: CtbSizeY / 2 x CtbSizeY);
    params = structured (CTB rows, CTB columns) array of SAO_CTB_DTYPE; keep = one byte per 8x8 samples (non-zero: left as
    is); a sample whose edge-offset neighbour lies outside the picture is left as is.  Returns a new array."""
    src = np.asarray(plane, np.int64)
    h, w = src.shape
    max_v = (1 << bit_depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    P = np.asarray(params, SAO_CTB_DTYPE)
    ci = (yy >> ctb_log2_h) * P.shape[1] + (xx >> ctb_log2_w)  # the CTB of every sample
    flat = P.ravel()
    typ, cls = flat["type"].astype(np.int64)[ci], flat["cls"].astype(np.int64)[ci]
    offs = flat["offset"].astype(np.int64)  # SaoOffsetVal[1..4] per CTB
    # band offset: bandTable[(k + sao_band_position) & 31] = k + 1
    band = src >> (bit_depth - 5)
    k = (band - cls) & 31
    band_idx = np.where(k < 4, k + 1, 0)
    # edge offset: hPos / vPos of Table 8-13
    pad = np.pad(src, 1, constant_values=-1)
    inside = np.pad(np.ones((h, w), bool), 1, constant_values=False)
    hv = {0: ((0, -1), (0, 1)), 1: ((-1, 0), (1, 0)), 2: ((-1, -1), (1, 1)), 3: ((-1, 1), (1, -1))}
    edge_idx = np.zeros((h, w), np.int64)
    for c, ((ay, ax), (by, bx)) in hv.items():
        a = pad[1 + ay:1 + ay + h, 1 + ax:1 + ax + w]
        b = pad[1 + by:1 + by + h, 1 + bx:1 + bx + w]
        ok = inside[1 + ay:1 + ay + h, 1 + ax:1 + ax + w] & inside[1 + by:1 + by + h, 1 + bx:1 + bx + w]
        e = 2 + np.sign(src - a) + np.sign(src - b)
        e = np.where(e <= 2, np.where(e == 2, 0, e + 1), e)  # edgeIdx 0, 1, 2 -> 1, 2, 0
        edge_idx = np.where((cls == c) & ok, e, np.where(cls == c, 0, edge_idx))
    idx = np.where(typ == 1, band_idx, np.where(typ == 2, edge_idx, 0))
    res = np.clip(src + np.where(idx > 0, offs[ci, np.maximum(idx - 1, 0)], 0), 0, max_v)
    if keep is not None:
        kept = np.asarray(keep)[yy >> 3, xx >> 3] != 0
        res = np.where(kept, src, res)
    return res.astype(np.asarray(plane).dtype)


def random_sao_params(w, h, ctb_log2_w, ctb_log2_h, rng, bit_depth=8):
    """random parameters for a w x h plane with (1 << ctb_log2_w) x (1 << ctb_log2_h) CTBs; edge offsets signed as 7.4.9.3.2"""
    rows, cols = -(-h >> ctb_log2_h), -(-w >> ctb_log2_w)
    p = np.zeros((rows, cols), SAO_CTB_DTYPE)
    p["type"] = rng.integers(0, 3, (rows, cols))
    band = p["type"] == 1
    p["cls"] = np.where(band, rng.integers(0, 32, (rows, cols)), rng.integers(0, 4, (rows, cols)))
    lim = (1 << (min(bit_depth, 10) - 5)) - 1
    off = rng.integers(-lim, lim + 1, (rows, cols, 4))
    if bit_depth > 10:  # log2OffsetScale 0 .. Max(0, bitDepth - 10), as far as the int8 entry holds the scaled value
        off = off << rng.integers(0, min(bit_depth - 10, 2) + 1, (rows, cols, 1))
    eo = ~band
    off[eo, 0:2] = np.abs(off[eo, 0:2])
    off[eo, 2:4] = -np.abs(off[eo, 2:4])
    p["offset"] = off
    return p
