"""SAO and deblocking + SAO of a semi-planar chroma plane (one plane of interleaved Cb / Cr pairs, the _sp SAO entries): what is
expected, the vectors, and the census that keeps a test from passing vacuously.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED like the rest of the spec-exact mode.  There is NO new filter logic here: the expectation is
  split the pairs (tests/sp_ref.py),
  tests/g4_ref.py sao_direct per component with THAT component's parameters and the common keep map and layout,
  interleave;
the chain is sp_ref.deblock followed by that.  A plane is an array (plane_h, plane_w, 2): [..., 0] the even samples of a row.

The kernels' geometry is the one the shapes below assume: a wave covers 64 x 64 pairs, a workgroup a strip of 256 x 64."""
import numpy as np

import g4_ref as G
import sao_borders_ref as B
import sp_ref as S

FRAMES = 5   # border_params rotates every border CTB through the four edge classes and the band offset

# (name, samples per component across, down, bit depth, ctb_log2)
VECTORS = [("16x16", 16, 16, 8, 3),            # one partial wave, every block on the border
           ("12x12", 12, 12, 8, 3),            # the smallest g4 plane: blocks of 4 columns and of 4 rows
           ("136x136", 136, 136, 8, 5),        # the smallest plane with an interior wave (region 64..127 both ways)
           ("140x132", 140, 132, 8, 4),        # g4 in both directions with an interior wave
           ("264x136_10", 264, 136, 10, 5),    # two strips per row, interior waves, the packed 16-bit kernel
           ("140x132_12", 140, 132, 12, 4),    # g4 at 16 bit
           ("72x24_14", 72, 24, 14, 3)]        # the per-sample kernel
CHAIN = ["136x136", "140x132_12"]


def rx_dtype():
    import rext_oracle as rx
    return rx.SAO_CTB_DTYPE


def spec_of(name):
    return next(s for s in VECTORS if s[0] == name)


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def sao(plane, pcb, pcr, lg, depth, keep=None, layout=None):
    cb, cr = S.split(plane)
    return S.merge(G.sao_direct(cb, pcb, lg, lg, bit_depth=depth, keep=keep, layout=layout),
                   G.sao_direct(cr, pcr, lg, lg, bit_depth=depth, keep=keep, layout=layout))


def expected(c, f, keep=False, layout=None, swap=False):
    pcb, pcr = (c["pcr"][f], c["pcb"][f]) if swap else (c["pcb"][f], c["pcr"][f])
    return sao(c["planes"][f], pcb, pcr, c["lg"], c["depth"], keep=c["keep"][f] if keep else None, layout=layout)


# ---- the vectors -------------------------------------------------------------------------------------------------------------------

def _own_offsets(p):
    """offsets of a component of its own, never zero: magnitudes + 1, signed as an edge offset (+ + - -) or alternating for a band"""
    m = np.minimum(np.abs(p["offset"].astype(np.int64)) + 1, 127)
    edge = (p["type"] == 2)[..., None]
    p["offset"] = np.where(edge, m * np.array([1, 1, -1, -1]), m * np.array([1, -1, 1, -1]))


def _constrain(pcb, pcr, f, rng):
    """Cr takes Cb's type and class everywhere (7.3.8.3: one SaoTypeIdx, one SaoEoClass per CTB) with its own offsets and band
    position; then two CTBs of the frame are made to disagree -- one in type, one in class with both edge offset -- or, on a grid of
    at most four CTBs, one of the two kinds in turn (so that more than half of the CTBs still agree)"""
    rows, cols = pcb.shape
    n = rows * cols
    was_band = pcr["type"] == 1
    pcr["type"] = pcb["type"]
    band = pcb["type"] == 1
    pcr["cls"] = np.where(band, np.where(was_band, pcr["cls"], (pcb["cls"].astype(np.int64) + 5) & 31), pcb["cls"])
    flat_b, flat_r = pcb.reshape(-1), pcr.reshape(-1)
    d1 = f % n
    both = n > 4
    if both or f % 2 == 0:   # the types differ
        if flat_b["type"][d1] == 2:
            flat_r["type"][d1], flat_r["cls"][d1] = 1, int(rng.integers(0, 32))
        else:
            flat_r["type"][d1], flat_r["cls"][d1] = 2, f % 4
    if both or f % 2 == 1:   # both edge offset, another class
        for k in range(n):
            d2 = (f + 1 + k) % n
            if (d2 != d1 or not both) and flat_b["type"][d2] == 2:
                flat_r["type"][d2], flat_r["cls"][d2] = 2, (int(flat_b["cls"][d2]) + 1 + f % 3) & 3
                break
    _own_offsets(pcr)


def case(spec):
    name, w, h, depth, lg = spec
    rng = np.random.default_rng(G.seed_of("saosp" + name))
    planes = [S.merge(G.noise_plane(w, h, depth, rng), G.noise_plane(w, h, depth, rng)) for _ in range(FRAMES)]
    pcb = G.border_params(w, h, lg, lg, depth, FRAMES, rng)
    pcr = G.border_params(w, h, lg, lg, depth, FRAMES, rng)
    for f in range(FRAMES):
        _constrain(pcb[f], pcr[f], f, rng)
    G.fit_bands([p[..., 0] for p in planes], pcb, lg, lg, depth)
    G.fit_bands([p[..., 1] for p in planes], pcr, lg, lg, depth)
    c = {"name": name, "w": w, "h": h, "depth": depth, "sb": 1 if depth == 8 else 2, "lg": lg, "planes": planes, "pcb": pcb, "pcr": pcr,
         "params": pcb, "keep": [G.keep_map(w, h, rng) for _ in range(FRAMES)]}
    # the "mixed" layout of g4_ref.sao_layout; on a grid of a few CTBs the first draw may forbid nothing: the next that does
    for seed in range(16):
        c["layout"] = G.sao_layout(c, seed)
        if B.expected_nox(c["layout"]).any():
            break
    return c


def chain_case(spec, frames=2):
    """blocky pair planes with bS, a QP map and per-slice pairs (sp_ref.dbk_case) and the SAO operands of case(spec)"""
    d = S.dbk_case(spec[:4], frames=frames)
    c = case(spec)
    d.update({k: c[k] for k in ("lg", "pcb", "pcr", "params", "keep", "layout")})
    return d


def chain_expected(c, f, sl, layout):
    dbk = S.dbk_expected(c, f, True, sl)
    return dbk, sao(dbk, c["pcb"][f], c["pcr"][f], c["lg"], c["depth"], keep=c["keep"][f], layout=layout)


# ---- the census ------------------------------------------------------------------------------------------------------------------

def census(c):
    w, h, lg, depth = c["w"], c["h"], c["lg"], c["depth"]
    yy, xx = np.mgrid[0:h, 0:w]
    cen = {"changed": [{k: 0 for k in ("e0", "e1", "e2", "e3", "band")} for _ in range(2)], "swap": [0, 0], "kept": 0, "layout": 0,
           "agree": 0, "types_differ": 0, "classes_differ": 0, "ctbs": 0, "g4": [None, None]}
    for f in range(FRAMES):
        want, other = expected(c, f), expected(c, f, swap=True)
        for k, p in enumerate((c["pcb"][f], c["pcr"][f])):
            typ, cls = p["type"][yy >> lg, xx >> lg], p["cls"][yy >> lg, xx >> lg]
            ch = want[..., k] != c["planes"][f][..., k]
            for e in range(4):
                cen["changed"][k]["e%d" % e] += int((ch & (typ == 2) & (cls == e)).sum())
            cen["changed"][k]["band"] += int((ch & (typ == 1)).sum())
            cen["swap"][k] += int((want[..., k] != other[..., k]).sum())
        kept = expected(c, f, keep=True)
        mask = np.repeat(np.repeat(c["keep"][f], 8, 0), 8, 1)[:h, :w].astype(bool)
        assert np.array_equal(kept[mask], c["planes"][f][mask])
        cen["kept"] += int((want[mask] != c["planes"][f][mask]).sum())
        cen["layout"] += int((expected(c, f, layout=c["layout"]) != want).sum())
        b, r = c["pcb"][f], c["pcr"][f]
        same_t = b["type"] == r["type"]
        same = same_t & ((b["type"] != 2) | (b["cls"] == r["cls"]))
        cen["agree"] += int(same.sum())
        cen["types_differ"] += int((~same_t).sum())
        cen["classes_differ"] += int((same_t & (b["type"] == 2) & (b["cls"] != r["cls"])).sum())
        cen["ctbs"] += b.size
    if G.is_g4(w, h):
        for k, key in enumerate(("pcb", "pcr")):
            cen["g4"][k] = G.sao_census([p[..., k] for p in c["planes"]], c[key], lg, lg, depth)
    return cen


def census_ok(c, cen):
    for k in range(2):
        if not all(v > 0 for v in cen["changed"][k].values()) or not cen["swap"][k] > 0:
            return False
        if cen["g4"][k] is not None and not G.census_ok(cen["g4"][k], c["w"], c["h"]):
            return False
    return (cen["kept"] > 0 and cen["layout"] > 0 and 2 * cen["agree"] > cen["ctbs"] and cen["types_differ"] > 0 and
            cen["classes_differ"] > 0)
