"""Semi-planar chroma (one plane of interleaved Cb / Cr pairs, the _sp entry): what is expected, the vectors, and the census that
keeps a test from passing vacuously.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED like the rest of the spec-exact mode.  There is NO new filter logic here: the expectation is
the existing statements applied per component --
  split the pairs,
  deblocking   tests/rext_oracle.py filter_chroma_plane with that component's cQpPicOffset (tests/g4_ref.py deblock_direct), or the
               composition of tests/slice_offsets_ref.py for per-slice pairs (g4_ref.deblock_sl),
  interleave the results.
A plane is an array (plane_h, plane_w, 2): [..., 0] the even samples of a row (Cb in NV12 order), [..., 1] the odd ones."""
import numpy as np

import g4_ref as G
import slice_offsets_ref as R

QP, CB_OFF, CR_OFF, TC_DIV2 = 37, -6, 6, 1
UNIT_LOG2, SL_CTB_LOG2 = G.UNIT_LOG2, G.SL_CTB_LOG2


def split(p):
    p = np.asarray(p)
    return np.ascontiguousarray(p[..., 0]), np.ascontiguousarray(p[..., 1])


def merge(cb, cr):
    return np.ascontiguousarray(np.stack([cb, cr], axis=-1))


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def deblock(plane, vb, hb, *, qp, qp_map=None, unit_log2=UNIT_LOG2, bit_depth=8, cb_qp_offset=0, cr_qp_offset=0, tc_offset_div2=0,
            slice_pairs=None, sl_ctb_log2=SL_CTB_LOG2):
    """8.7.2 of both components; slice_pairs = (rows, cols, 2) of the LUMA CTB grid (then tc_offset_div2 is not used)"""
    out = []
    for comp, off in zip(split(plane), (cb_qp_offset, cr_qp_offset)):
        kw = dict(qp=qp, qp_map=qp_map, unit_log2=unit_log2, bit_depth=bit_depth, c_qp_offset=off)
        if slice_pairs is None:
            out.append(G.deblock_direct(comp, vb, hb, 1, tc_offset_div2=tc_offset_div2, **kw))
        else:
            out.append(G.deblock_sl(comp, vb, hb, 1, slice_pairs, sl_ctb_log2, **kw))
    return merge(*out)


# ---- deblocking vectors ------------------------------------------------------------------------------------------------------------

# (name, samples per component across, down, bit depth): the smallest shapes at which each path of the kernels can go wrong
DBK = [("16x16", 16, 16, 8),          # one partial wave: first and last block row, first and last lane
       ("12x12", 12, 12, 8),          # the smallest g4 plane
       ("1032x24", 1032, 24, 8),      # nbx = 130: a first wave, one INTERIOR wave, a last wave; two interior block rows
       ("1032x24_10", 1032, 24, 10),
       ("1028x20", 1028, 20, 8),      # g4 in both directions with an interior wave
       ("36x36_10", 36, 36, 10),      # g4 in both directions without one
       ("72x24_14", 72, 24, 14)]      # deeper than 12 bit: the 32-bit kernel


def dbk_case(spec, frames=2):
    """`frames` blocky pair planes with per-frame bS, a QP map per 8 x 8 luma samples, per-slice pairs (slices of three CTBs)"""
    name, w, h, depth = spec
    rng = np.random.default_rng(G.seed_of("sp" + name))
    rows, cols = -(-2 * h >> SL_CTB_LOG2), -(-2 * w >> SL_CTB_LOG2)
    sidx = R.slices_raster(rows, cols, 3)
    return {"name": name, "w": w, "h": h, "depth": depth, "sb": 1 if depth == 8 else 2, "qp": QP,
            "planes": [merge(G.blocky_plane(w, h, depth, rng), G.blocky_plane(w, h, depth, rng)) for _ in range(frames)],
            "bs": [G.random_bs(w, h, rng) for _ in range(frames)],
            "qp_map": G.random_qp_map(w, h, 1, UNIT_LOG2, rng, lo=30, hi=42),
            "pairs": R.ctb_pairs(sidx, R.table_for(int(sidx.max()) + 1))}


def dbk_expected(c, f, qmap, sl, swap=False, src=None):
    """frame f: one QP (qmap False) or the map; the call's own tc offset, or per-slice pairs (sl True); swap: the two cQpPicOffsets
    exchanged (what a kernel that confused the components would compute)"""
    vb, hb = c["bs"][f]
    cb, cr = (CR_OFF, CB_OFF) if swap else (CB_OFF, CR_OFF)
    return deblock(c["planes"][f] if src is None else src, vb, hb, qp=c["qp"], qp_map=c["qp_map"] if qmap else None, bit_depth=c["depth"],
                   cb_qp_offset=cb, cr_qp_offset=cr, tc_offset_div2=TC_DIV2, slice_pairs=c["pairs"] if sl else None)


def dbk_census(c, f, qmap, sl, want=None):
    """what frame f's expectation exercises, per component: samples changed; samples at which the expectation with the two offsets
    exchanged differs; samples changed at the new last edges of a g4 plane (0 for a direction that is a multiple of 8)"""
    want = dbk_expected(c, f, qmap, sl) if want is None else want
    other = dbk_expected(c, f, qmap, sl, swap=True)
    cen = []
    for k in range(2):
        src = c["planes"][f][..., k]
        cols, rows = G.new_edge_changes(src, want[..., k])
        cen.append({"changed": int((want[..., k] != src).sum()), "swap": int((want[..., k] != other[..., k]).sum()),
                    "new_cols": cols, "new_rows": rows})
    return cen


def dbk_census_ok(c, cen):
    for k in range(2):
        if not (cen[k]["changed"] > 0 and cen[k]["swap"] > 0):
            return False
        if c["w"] % 8 and not cen[k]["new_cols"] > 0:
            return False
        if c["h"] % 8 and not cen[k]["new_rows"] > 0:
            return False
    return True
