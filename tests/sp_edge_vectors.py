"""Pair-plane vectors (one plane of interleaved Cb / Cr pairs, the _sp entries) at the decision edges, over the full sample range and
over every boundary byte: the vectors of tests/h265_vectors.py and tests/sao_bytes_vectors.py, which the planar kernels are pinned by,
made for two components that share one plane, one set of bS entries, one QP map, one keep map and one byte array.

TEST INFRASTRUCTURE ONLY.  There is NO filter logic here.  What is expected of a vector is the existing statements applied per
component: sp_ref.deblock, rext_oracle.sao_plane / sao_borders_ref.sao_plane_by_bytes, and the chain of the two.  The censuses are
h265_vectors.chroma_events and h265_vectors.sao_census per component.

A plane is an array (h, w, 2): [..., 0] the even samples of a row (Cb in NV12 order), [..., 1] the odd ones."""
import functools
from collections import Counter

import numpy as np

import g4_ref as G
import h265_vectors as hv
import rext_oracle as rx
import sao_borders_ref as B
import sao_bytes_vectors as V
import slice_offsets_ref as R
import sp_ref as S

UNIT_LOG2, SL_CTB_LOG2 = S.UNIT_LOG2, S.SL_CTB_LOG2
EVENTS = ("tc_clip_lo", "tc_clip_hi", "clip1_p0_lo", "clip1_p0_hi", "clip1_q0_lo", "clip1_q0_hi")


# ---- deblocking --------------------------------------------------------------------------------------------------------------------

def _segment(case, tc, max_v, rng):
    """the 4 x 8 samples p3..q3 of one component of one segment: the four cases of h265_vectors._chroma_plane, fitted to tc"""
    if case == 0:    # |delta| beyond tC: delta = ((q0 - p0) * 4 + p1 - q1 + 4) >> 3 with a plain step
        g = min(max(2 * tc + 2, 4) + int(rng.integers(0, 4 * max(tc, 1) + 1)), max_v)
        base = int(rng.integers(0, max_v - g + 1))
        ln = [base] * 4 + [base + g] * 4
    elif case == 1:  # Clip1: p0 at the bottom, the Q side rising steeply
        c = int(rng.integers(0, max(tc, 1)))
        s = min(int(rng.integers(8 * max(tc, 1), max(8 * max(tc, 1), max_v // 3) + 1)), max_v // 3)
        ln = [c] * 4 + [0, s, 2 * s, 3 * s]
    elif case == 2:  # small steps: delta inside +-tC
        g = int(rng.integers(-max(tc, 1), max(tc, 1) + 1))
        base = int(rng.integers(abs(g), max_v - abs(g) + 1))
        ln = [base] * 4 + [base + g] * 4
    else:            # a step over the full range
        ln = [0] * 4 + [max_v] * 4
    seg = np.clip(np.array([ln] * 4, np.int64) + rng.integers(0, 2, (4, 8)), 0, max_v)
    if rng.integers(0, 2):
        seg = max_v - seg
    if rng.integers(0, 2):
        seg = seg[:, ::-1]
    return seg


def dbk_pair_plane(depth, rng, w, h, *, qp, qp_map, cb_off, cr_off, tc_div2, slice_pairs=None, direction="v"):
    """A pair plane of w x h samples per component (multiples of 4, at least 8) whose vertical (or, "h", horizontal) edge segments put
    the chroma filter (8.7.2.5.8) of BOTH components at its ends.  The bS entry of a segment (bS 0 / 1 / 2, KEEP_P / KEEP_Q) is drawn
    once for both components; the content of each component is fitted to that component's own tC -- rext_oracle.chroma_tc with its
    cQpPicOffset and, with slice_pairs ((rows, cols, 2) of the luma CTB grid of 1 << SL_CTB_LOG2), the tc offset of the CTB holding
    q0,0 as slice_offsets_ref states it, added to tc_div2 -- and component k of segment n takes case (n + k) % 4 of
    h265_vectors._chroma_plane, so that the two components of a segment are never in the same case.  The new last edge of a size
    that is no multiple of 8 gets segments like any other.  Returns plane (h, w, 2), vb, hb (the other direction all 0)."""
    if direction == "h":
        m = None if qp_map is None else np.ascontiguousarray(np.asarray(qp_map).T)
        sp = None if slice_pairs is None else np.ascontiguousarray(np.asarray(slice_pairs).transpose(1, 0, 2))
        p, vb, _ = dbk_pair_plane(depth, rng, h, w, qp=qp, qp_map=m, cb_off=cb_off, cr_off=cr_off, tc_div2=tc_div2, slice_pairs=sp)
        vbT = vb.reshape(w // 4, h // 8 + 1)
        return np.ascontiguousarray(p.transpose(1, 0, 2)), np.zeros(G.num_vert_bs(w, h), np.uint8), np.ascontiguousarray(vbT.T).ravel()
    assert w % 4 == 0 and h % 4 == 0 and w >= 8 and h >= 8
    max_v = (1 << depth) - 1
    plane = rng.integers(max_v // 4, 3 * max_v // 4 + 1, (h, w, 2)).astype(np.int64)
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    m = None if qp_map is None else np.asarray(qp_map, np.int64)
    lw, lh = 2 * w, 2 * h
    n = 0
    for y4 in range(h // 4):
        for bx in range(1, (w + 7) // 8):
            x = 8 * bx
            r = int(rng.integers(0, 16))
            ent = 0 if r == 0 else 1 if r == 1 else 2
            if rng.integers(0, 10) == 0:
                ent |= (hv.KEEP_P, hv.KEEP_Q)[int(rng.integers(0, 2))]
            vb[y4, bx] = ent
            if m is None:
                qpl = min(int(qp), 51)
            else:
                def at(cx, cy):
                    return int(m[min(cy * 2, lh - 1) >> UNIT_LOG2, min(cx * 2, lw - 1) >> UNIT_LOG2])
                qpl = min((at(x, 4 * y4) + at(x - 1, 4 * y4) + 1) >> 1, 51)
            t = tc_div2
            if slice_pairs is not None:
                t += int(slice_pairs[min(8 * y4, lh - 1) >> SL_CTB_LOG2, min(2 * x, lw - 1) >> SL_CTB_LOG2, 1])
            for k, off in enumerate((cb_off, cr_off)):
                tc = int(rx.chroma_tc(qpl, 1, c_qp_offset=off, tc_offset_div2=t, bit_depth=depth))
                plane[4 * y4:4 * y4 + 4, x - 4:x + 4, k] = _segment((n + k) % 4, tc, max_v, rng)
            n += 1
    return plane.astype(np.uint8 if depth == 8 else np.uint16), vb.ravel(), np.zeros(G.num_hor_bs(w, h), np.uint8)


# (name, qp, cb_qp_offset, cr_qp_offset, tc_offset_div2): qp None = h265_vectors.all_qp_map 0..51; "slices" = per-slice pairs drawn
# from SLICE_VALUES with the call's own beta / tC offsets 0 (the per-slice operand replaces them)
OPERANDS = [("q51", 51, 12, -12, 6),      # qPi 63 and 39: Q = QpC + 2 + 12 clipped to 53 for the even samples
            ("q0", 0, -12, 12, -6),       # qPi -12 and 12: Q = 0 and 2, tC = 0 -- nothing may change
            ("q36", 36, -7, -6, 0),       # qPi 29 and 30: below and at the first knee of Table 8-10
            ("q37", 37, 6, 7, 0),         # qPi 43 and 44: at and above the last knee
            ("q20", 20, -3, 3, -1),       # tC 0 for one component, 1 for the other
            ("allqp", None, -5, 9, 1),
            ("slices", 30, 9, -8, 0)]
SLICE_VALUES = (-6, -1, 0, 1, 6)
FRAMES = ("v", "h", "both")   # vertical vectors, the transposed twin, the vertical vectors under random horizontal bS entries


def operand(name):
    return next(o for o in OPERANDS if o[0] == name)


@functools.lru_cache(maxsize=None)
def dbk_case(spec, op_name):
    """three frames of one shape of sp_ref.DBK under one operand set, in the form tests/test_gpu_sp.py PairPlane takes"""
    name, w, h, depth = spec
    _, qp, cb, cr, tcd = operand(op_name)
    rng = np.random.default_rng(G.seed_of("spedge" + name + op_name))
    qmap = None
    if qp is None:   # every QP 0..51; a plane of fewer than 52 units takes the highest ones, where tC is not 0
        units = (-(-2 * h >> UNIT_LOG2)) * (-(-2 * w >> UNIT_LOG2))
        qmap = hv.all_qp_map(2 * w, 2 * h, UNIT_LOG2, rng, lo=max(0, 52 - units))
    pairs = None
    if op_name == "slices":
        rows, cols = -(-2 * h >> SL_CTB_LOG2), -(-2 * w >> SL_CTB_LOG2)
        sidx = R.slices_raster(rows, cols, 3)
        table = rng.choice(SLICE_VALUES, (int(sidx.max()) + 1, 2)).astype(np.int8)
        table[: len(SLICE_VALUES), 1] = SLICE_VALUES[: table.shape[0]]     # every tC offset, as far as there are slices
        pairs = R.ctb_pairs(sidx, table)
    kw = dict(qp=qp or 0, qp_map=qmap, cb_off=cb, cr_off=cr, tc_div2=tcd, slice_pairs=pairs)
    planes, bs = [], []
    for d in ("v", "h", "v"):
        p, vb, hb = dbk_pair_plane(depth, rng, w, h, direction=d, **kw)
        planes.append(p)
        bs.append((vb, hb))
    bs[2] = (bs[2][0], G.random_bs(w, h, rng)[1])
    c = {"name": name + "/" + op_name, "shape": name, "op": op_name, "w": w, "h": h, "depth": depth, "sb": 1 if depth == 8 else 2,
         "qp": qp or 0, "cb": cb, "cr": cr, "tc_div2": tcd, "planes": planes, "bs": bs, "qp_map": qmap, "pairs": pairs}
    for a in planes + [x for b in bs for x in b]:
        a.setflags(write=False)
    return c


def dbk_deblock(c, plane, f, swap=False):
    vb, hb = c["bs"][f]
    cb, cr = (c["cr"], c["cb"]) if swap else (c["cb"], c["cr"])
    return S.deblock(plane, vb, hb, qp=c["qp"], qp_map=c["qp_map"], bit_depth=c["depth"], cb_qp_offset=cb, cr_qp_offset=cr,
                     tc_offset_div2=c["tc_div2"], slice_pairs=c["pairs"])


_dbk_wants = {}


def dbk_expected(c, f):
    """sp_ref.deblock of frame f, computed once"""
    key = (c["name"], f)
    if key not in _dbk_wants:
        _dbk_wants[key] = dbk_deblock(c, c["planes"][f], f)
        _dbk_wants[key].setflags(write=False)
    return _dbk_wants[key]


def dbk_events(c, f, k):
    """h265_vectors.chroma_events of component k of frame f (0: the vertical edges, 1: the horizontal edges, transposed); with
    per-slice pairs, one call per tC offset on the entries of the CTBs that own it"""
    assert f in (0, 1)
    w, h = c["w"], c["h"]
    plane, m, pairs = c["planes"][f][..., k], c["qp_map"], c["pairs"]
    if f == 0:
        vb = np.asarray(c["bs"][0][0]).reshape(h // 4, w // 8 + 1)
    else:
        plane = np.ascontiguousarray(plane.T)
        vb = np.ascontiguousarray(np.asarray(c["bs"][1][1]).reshape(h // 8 + 1, w // 4).T)
        m = None if m is None else np.ascontiguousarray(m.T)
        pairs = None if pairs is None else pairs.transpose(1, 0, 2)
    kw = dict(bit_depth=c["depth"], qp=c["qp"], qp_map=m, unit_log2=UNIT_LOG2, c_qp_offset=(c["cb"], c["cr"])[k])
    if pairs is None:
        return hv.chroma_events(plane, vb.ravel(), 1, tc_offset_div2=c["tc_div2"], **kw)
    ch, cw = plane.shape
    y4, bx = np.mgrid[0:vb.shape[0], 0:vb.shape[1]]
    own = pairs[np.minimum(8 * y4, 2 * ch - 1) >> SL_CTB_LOG2, np.minimum(16 * bx, 2 * cw - 1) >> SL_CTB_LOG2, 1]
    ev = Counter()
    for t in np.unique(own):
        ev.update(hv.chroma_events(plane, np.where(own == t, vb, 0).ravel(), 1, tc_offset_div2=c["tc_div2"] + int(t), **kw))
    return ev


def dbk_census(c):
    """per component: the events of the vertical and of the horizontal frame, the samples each frame changes, and the samples at which
    the expectation with the two cQpPicOffsets exchanged differs"""
    cen = []
    for k in range(2):
        d = {"v": dbk_events(c, 0, k), "h": dbk_events(c, 1, k), "changed": [], "swap": 0, "new_cols": 0, "new_rows": 0}
        for f in range(3):
            want = dbk_expected(c, f)
            d["changed"].append(int((want[..., k] != c["planes"][f][..., k]).sum()))
            d["swap"] += int((want[..., k] != dbk_deblock(c, c["planes"][f], f, swap=True)[..., k]).sum())
            cols, rows = G.new_edge_changes(c["planes"][f][..., k], want[..., k])
            d["new_cols"] += cols
            d["new_rows"] += rows
        cen.append(d)
    return cen


def tc_of(c, k, qpl, slice_tc=0):
    """tC' index Q and tC of component k at (QpQ + QpP + 1) >> 1 = qpl"""
    qpc = int(rx.chroma_qp(qpl + (c["cb"], c["cr"])[k], 1))
    return qpc + 2 + 2 * (c["tc_div2"] + slice_tc), int(rx.chroma_tc(qpl, 1, c_qp_offset=(c["cb"], c["cr"])[k],
                                                                    tc_offset_div2=c["tc_div2"] + slice_tc, bit_depth=c["depth"]))


# ---- SAO ---------------------------------------------------------------------------------------------------------------------------

TILE_ROWS = (63, 64, 127, 128)   # the SAO wave's rows and the fused tile's rows


def border_cols(sb, w):
    """the columns (of pairs) on both sides of the semi-planar kernels' borders: the SAO wave (64) and strip (256), the fused tile of
    96 pairs (8-bit samples) or of 64 (16-bit containers)"""
    cols = {63, 64, 255, 256} | ({95, 96, 191, 192} if sb == 1 else {x for b in range(64, w, 64) for x in (b - 1, b)})
    return tuple(sorted(x for x in cols if x < w))


def _component(depth, lg, rng, w, h, cols, rows, walk_start):
    """h265_vectors.sao_full_range for a size in multiples of 4: made at the next multiple of 8 and cut"""
    p, prm, keep = hv.sao_full_range(depth, lg, rng, w=G.pad8(w), h=G.pad8(h), stripe_cols=cols, stripe_rows=rows, walk_start=walk_start)
    return np.ascontiguousarray(p[:h, :w]), prm, keep


def _edge_signed(off):
    o = np.minimum(np.abs(off.astype(np.int64)), 127)
    return o * np.array([1, 1, -1, -1])


def sao_pair_full_range(depth, lg, rng, w, h, tile_cols, tile_rows, walk_start=0):
    """Two h265_vectors.sao_full_range components (content over the full range, 0 next to max_v across tile_cols / tile_rows, offsets
    at the spec-legal scaled limits and at -128 / 127, every band position), merged.  The odd samples' parameters take the even
    samples' type and class in two CTBs of three (their own band position and their own offsets) and differ in the third: in type,
    or -- both edge offset -- in class, in turn (the rule of sao_sp_ref._constrain: the short and the general path of the packed
    kernels).  walk_start: h265_vectors.sao_full_range's, for both components.  Returns plane (h, w, 2), params of the even samples, of the odd samples, keep (one byte per 8 x 8, by ceiling)."""
    a, pa, keep = _component(depth, lg, rng, w, h, tile_cols, tile_rows, walk_start)
    b, pb, _ = _component(depth, lg, rng, w, h, tile_cols, tile_rows, walk_start)
    fa, fb = pa.reshape(-1), pb.reshape(-1)
    turn = int(rng.integers(0, 6))
    for i in range(fa.size):
        ta, was = int(fa["type"][i]), int(fb["type"][i])
        if i % 3 != 2:        # agree
            fb["type"][i] = ta
            if ta == 2:
                fb["cls"][i] = fa["cls"][i]
            elif ta == 1 and was != 1:
                fb["cls"][i] = (int(fa["cls"][i]) + 5) & 31
        elif ta == 2 and turn % 2 == 0:   # both edge offset, another class
            fb["type"][i], fb["cls"][i] = 2, (int(fa["cls"][i]) + 1 + turn // 2 % 3) & 3
            turn += 1
        else:                 # another type
            if ta == 2:
                fb["type"][i], fb["cls"][i] = 1, int(rng.integers(0, 32))
            else:
                fb["type"][i], fb["cls"][i] = 2, i % 4
            turn += 1
        if fb["type"][i] == 2 and was != 2:
            fb["offset"][i] = _edge_signed(fb["offset"][i])
    return S.merge(a, b), pa, pb, keep


# (name, samples per component across, down, bit depth, ctb_log2)
SAO = [("264x136", 264, 136, 8, 5),        # two strips, interior waves, three fused tiles across and two down
       ("264x136_10", 264, 136, 10, 3),    # the packed 16-bit kernels, five fused tiles across; the smallest CTBs
       ("140x132", 140, 132, 8, 4),        # g4 in both directions
       ("140x132_12", 140, 132, 12, 4),    # g4 at 16 bit; offsets scaled by 1 << 2
       ("12x12", 12, 12, 8, 3),
       ("72x24_14", 72, 24, 14, 3)]        # the per-sample kernel
SAO_FRAMES = 2   # of the shapes with an interior wave
# The two small shapes have few CTBs per frame (4 and 27), and sao_full_range begins its walk through the band positions
# (13 * n % 32 for the n-th band CTB) and the offset magnitudes anew with every call.  They get six frames whose walks begin where
# the positions 29, 30 and 31 (n = 17, 22, 27: the bands that wrap, band 31 among them) and the -128 / 127 turn come up at once.
SMALL_WALKS = (0, 17, 22, 27, 49, 59)
FUSED = ["264x136", "264x136_10", "140x132", "140x132_12"]


def sao_spec(name):
    return next(s for s in SAO if s[0] == name)


@functools.lru_cache(maxsize=None)
def sao_case(spec):
    """full-range pair planes (SAO_FRAMES of them, or one per entry of SMALL_WALKS) with per-frame parameters of both components,
    keep maps and ARBITRARY border bytes (per frame, a stride larger than the CTB columns)"""
    name, w, h, depth, lg = spec
    rng = np.random.default_rng(G.seed_of("saoedge" + name))
    sb = 1 if depth == 8 else 2
    cols = border_cols(sb, w)
    walks = (0,) * SAO_FRAMES if w >= 140 else SMALL_WALKS
    n = len(walks)
    fr = [sao_pair_full_range(depth, lg, rng, w, h, cols, TILE_ROWS, walk_start=ws) for ws in walks]
    r, c = fr[0][1].shape
    nox = np.full((n, r, c + V.STRIDE_EXTRA), V.NOX_POISON, np.uint8)
    nox[:, :, :c] = rng.integers(0, 256, (n, r, c))
    out = {"name": name, "w": w, "h": h, "depth": depth, "sb": sb, "lg": lg, "planes": [x[0] for x in fr], "pcb": [x[1] for x in fr],
           "pcr": [x[2] for x in fr], "keep": [x[3] for x in fr], "nox": nox, "cols": cols, "rows": tuple(y for y in TILE_ROWS if y < h)}
    for a in out["planes"] + out["pcb"] + out["pcr"] + out["keep"] + [nox]:
        a.setflags(write=False)
    return out


def sao(plane, pcb, pcr, lg, depth, keep=None, nox=None):
    """rext_oracle.sao_plane, or with bytes sao_borders_ref.sao_plane_by_bytes, per component"""
    out = []
    for comp, prm in zip(S.split(plane), (pcb, pcr)):
        if nox is None:
            out.append(rx.sao_plane(comp, prm, lg, lg, bit_depth=depth, keep=keep))
        else:
            out.append(B.sao_plane_by_bytes(comp, prm, lg, lg, nox, bit_depth=depth, keep=keep))
    return S.merge(*out)


_sao_wants = {}


def sao_expected(c, f, keep, borders):
    key = (c["name"], f, keep, borders)
    if key not in _sao_wants:
        _sao_wants[key] = sao(c["planes"][f], c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f] if keep else None,
                              nox=c["nox"][f] if borders else None)
        _sao_wants[key].setflags(write=False)
    return _sao_wants[key]


def sao_tags(c):
    """h265_vectors.sao_census per component, over the frames, without the keep map"""
    tags = [set(), set()]
    for f in range(len(c["planes"])):
        for k, key in enumerate(("pcb", "pcr")):
            tags[k] |= hv.sao_census(c["planes"][f][..., k], c[key][f], c["lg"], c["depth"])
    return tags


def sao_agreement(c):
    """(CTBs, CTBs whose type and class agree between the components, CTBs that differ in type, in class with both edge offset)"""
    n = same = types = classes = 0
    for b, r in zip(c["pcb"], c["pcr"]):
        st = b["type"] == r["type"]
        n += b.size
        same += int((st & ((b["type"] != 2) | (b["cls"] == r["cls"]))).sum())
        types += int((~st).sum())
        classes += int((st & (b["type"] == 2) & (b["cls"] != r["cls"])).sum())
    return n, same, types, classes


def sao_border_changes(c):
    """per component: {("col" | "row", index): samples changed there over the frames} for every column / row of c["cols"] / c["rows"]"""
    out = [Counter(), Counter()]
    for f in range(len(c["planes"])):
        d = sao_expected(c, f, False, False) != c["planes"][f]
        for k in range(2):
            for x in c["cols"]:
                out[k][("col", x)] += int(d[:, x, k].sum())
            for y in c["rows"]:
                out[k][("row", y)] += int(d[y, :, k].sum())
    return out


# ---- every boundary byte -----------------------------------------------------------------------------------------------------------

# name -> (bit depth, ctb_log2, CTB rows, CTB columns, frames, seed, samples cut from the last CTB column, row): the smallest sizes
# holding 1024 interior CTBs
BYTES = {"bytes_8b_ctb8": (8, 3, 34, 34, 1, 811, 0, 0), "bytes_10b_ctb16": (10, 4, 34, 34, 1, 812, 0, 0),
         "bytes_8b_ctb32": (8, 5, 18, 18, 4, 813, 0, 0), "bytes_8b_g4_ctb8": (8, 3, 34, 34, 1, 814, 4, 4)}


def every_byte_pairs(name, depth, lg, rows, cols, frames, seed, cut_w=0, cut_h=0):
    """sao_bytes_vectors.every_byte for a pair plane: ONE byte array for both components, the odd samples' interior classes the even
    samples' turned by one (as chroma_every_byte does), so that every (byte, class) pair sits on an interior CTB of each component"""
    a = V.every_byte(name + "_even", depth, lg, lg, rows, cols, frames, seed, cut_w=cut_w, cut_h=cut_h)
    b = V.every_byte(name + "_odd", depth, lg, lg, rows, cols, frames, seed + 100, cut_w=cut_w, cut_h=cut_h)
    for pb, pa in zip(b["params"], a["params"]):
        pb["cls"][1:-1, 1:-1] = (pa["cls"][1:-1, 1:-1] + 1) & 3
    c = {"name": name, "w": a["w"], "h": a["h"], "depth": depth, "sb": a["sb"], "lg": lg, "grid": (rows, cols),
         "planes": [S.merge(x, y) for x, y in zip(a["planes"], b["planes"])], "pcb": a["params"], "pcr": b["params"], "nox": a["nox"],
         "keep": [np.zeros(((a["h"] + 7) // 8, (a["w"] + 7) // 8), np.uint8) for _ in range(frames)]}
    for x in c["planes"] + c["pcb"] + c["pcr"] + [c["nox"]]:
        x.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def bytes_case(name):
    return every_byte_pairs(name, *BYTES[name])


@functools.lru_cache(maxsize=None)
def bytes_expected(name, f):
    c = bytes_case(name)
    out = sao(c["planes"][f], c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], nox=c["nox"][f])
    out.setflags(write=False)
    return out


def bytes_bs(c):
    """bS entries of all 0 for every frame: deblocking is the identity and the SAO stage of a fused kernel sees every byte"""
    return [(np.zeros(G.num_vert_bs(c["w"], c["h"]), np.uint8), np.zeros(G.num_hor_bs(c["w"], c["h"]), np.uint8)) for _ in c["planes"]]


# ---- deblocking + SAO ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain_case(name, op_name):
    """the deblocking vector of the shape under an operand set with the full-range SAO content of sao_case laid over every third
    16 x 16 block (as test_gpu_h265_boundaries.test_deblock_sao_single_plane does for luma), and sao_case's SAO operands"""
    sp = sao_spec(name)
    d = dbk_case(sp[:4], op_name)
    s = sao_case(sp)
    h, w = d["h"], d["w"]
    blk = ((np.arange(h)[:, None] // 16 + np.arange(w)[None, :] // 16) % 3 == 0)[..., None]
    c = dict(d)
    c["planes"] = [np.where(blk, s["planes"][f], d["planes"][f]).astype(d["planes"][f].dtype) for f in range(SAO_FRAMES)]
    c["bs"] = d["bs"][:SAO_FRAMES]
    c["name"] = "chain/" + d["name"]
    c.update({k: s[k] for k in ("lg", "pcb", "pcr", "keep", "nox")})
    return c


_chain_wants = {}


def chain_expected(c, f, borders):
    """(deblocked, final) of frame f with the keep map; borders: the arbitrary bytes"""
    key = (c["name"], f, borders)
    if key not in _chain_wants:
        dbk = dbk_deblock(c, c["planes"][f], f)
        _chain_wants[key] = (dbk, sao(dbk, c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f],
                                      nox=c["nox"][f] if borders else None))
    return _chain_wants[key]
