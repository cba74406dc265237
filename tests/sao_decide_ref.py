"""The SAO decision per CTB (hevcdbk_sao_decide_device, include/hevc_deblock.h): own parameters, merge left or merge up over Y, Cb
and Cr at once -- the rule stated serially, in raster order, in Python ints, on top of sao_stats_ref.pick_ctb / predicted_delta.

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of SAO.  Nothing of the library is mentioned here.  A grid is built from a
PALETTE: a few distinct statistics records (S_y, S_cb, S_cr) and a grid of indices into them.  What a CTB does depends on its record
and on the two candidate triples only, so the results are memoised by (record, triple) and grids of tens of thousands of CTBs stay
fast.  By construction a run of identical records along a row merges left (the same distortion for 1 bit against many, also when
NEW is "not applied"), vertical stripes merge up, and a change of record gives NEW.
"""
import numpy as np

import rext_oracle as ro
import sao_stats_ref as S

DECISION_DTYPE = np.dtype([("delta_d", "<i8"), ("cost_luma", "<i8"), ("cost_chroma", "<i8"), ("merge", "u1"), ("flag_bits", "u1"), ("cand", "u1"),
                           ("zero", "u1", (5,))])
assert DECISION_DTYPE.itemsize == 32
OFF = (0, 0, (0, 0, 0, 0))


def pick_cost(st_a, st_b, bit_depth, lam):
    """sao_stats_ref.pick_ctb and the least cost it found: (params per component, delta_d, cost).  The cost is the minimum over the
    candidates of the pick rule, enumerated here on their own"""
    out, dd = S.pick_ctb(st_a, st_b, bit_depth, lam)
    M = S.max_offset(bit_depth)
    comps = [S._bins(s, M, lam) for s in ((st_a,) if st_b is None else (st_a, st_b))]
    band = lambda c, p: sum(c[1][(p + j) & 31][1] for j in range(4))
    costs = [lam] + [lam * 4 + sum(b[1] for c in comps for b in c[0][k]) for k in range(4)]
    if st_b is None:
        costs += [lam * 7 + band(comps[0], p) for p in range(32)]
    else:
        costs.append(lam * 12 + sum(min(band(c, p) for p in range(32)) for c in comps))
    return out, dd, min(costs)


def pd(st, p):
    """the sum over the four bins the parameters p = (type, cls, offsets) use of n o^2 - 2 o s: sao_stats_ref.predicted_delta of one CTB"""
    one = np.zeros((1, 1), ro.SAO_CTB_DTYPE)
    one[0, 0] = p
    return int(S.predicted_delta(np.asarray(st).reshape(1, 1), one)[0, 0])


def candidates(cx, cy, slice_idx, tile_idx):
    def same(y, x):
        return (slice_idx is None or slice_idx[cy, cx] == slice_idx[y, x]) and (tile_idx is None or tile_idx[cy, cx] == tile_idx[y, x])
    return (1 if cx > 0 and same(cy, cx - 1) else 0) | (2 if cy > 0 and same(cy - 1, cx) else 0)


class Decider:
    """the rule for one set of depths and lambdas over one palette; decide() may be called for any number of grids"""

    def __init__(self, palette, *, bd_luma, lam_luma, bd_chroma=None, lam_chroma=None, chroma=True):
        self.palette, self.chroma = palette, chroma
        self.bd_l, self.lam_l = bd_luma, lam_luma
        self.bd_c, self.lam_c = bd_luma if bd_chroma is None else bd_chroma, lam_luma if lam_chroma is None else lam_chroma
        self._new, self._merge = {}, {}

    def J(self, c_y, c_c, F):
        if not self.chroma:
            return c_y + self.lam_l * F
        return self.lam_c * c_y + self.lam_l * c_c + self.lam_l * self.lam_c * F

    def new(self, k):
        """(triple, C_y, C_c, delta_d) of record k on its own"""
        if k not in self._new:
            sy, scb, scr = self.palette[k]
            (py,), dy, cy = pick_cost(sy, None, self.bd_l, self.lam_l)
            if self.chroma:
                (pcb, pcr), dc, cc = pick_cost(scb, scr, self.bd_c, self.lam_c)
            else:
                pcb, pcr, dc, cc = OFF, OFF, 0, 0
            self._new[k] = ((py, pcb, pcr), cy, cc, dy + dc)
        return self._new[k]

    def merged(self, k, triple):
        """(C_y, C_c) of record k under a neighbour's triple"""
        if (k, triple) not in self._merge:
            sy, scb, scr = self.palette[k]
            self._merge[(k, triple)] = (256 * pd(sy, triple[0]), 256 * (pd(scb, triple[1]) + pd(scr, triple[2])) if self.chroma else 0)
        return self._merge[(k, triple)]

    def decide(self, idx, slice_idx=None, tile_idx=None):
        """idx: (rows, cols) indices into the palette.  Returns {"params": [Y, Cb, Cr] (rows, cols) of SAO_CTB_DTYPE (Cb, Cr None without
        chroma), "decision": (rows, cols) of DECISION_DTYPE, "j": chosen J and "j_new": NEW's J per CTB, Python ints}"""
        rows, cols = idx.shape
        final = [[None] * cols for _ in range(rows)]
        dec = np.zeros((rows, cols), DECISION_DTYPE)
        j_of, j_new = np.zeros((rows, cols), object), np.zeros((rows, cols), object)
        for cy in range(rows):
            for cx in range(cols):
                k = int(idx[cy, cx])
                cand = candidates(cx, cy, slice_idx, tile_idx)
                triple, c_y, c_c, _ = self.new(k)
                F = (cand & 1) + (cand >> 1)
                best = (self.J(c_y, c_c, F), 0, triple, c_y, c_c, F)
                j_new[cy, cx] = best[0]
                for m, src in ((1, (cy, cx - 1)), (2, (cy - 1, cx))):
                    if not cand & m:
                        continue
                    t = final[src[0]][src[1]]
                    m_y, m_c = self.merged(k, t)
                    f = 1 if m == 1 else 1 + (cand & 1)
                    j = self.J(m_y, m_c, f)
                    if j < best[0]:
                        best = (j, m, t, m_y, m_c, f)
                j, m, t, c_y, c_c, F = best
                final[cy][cx] = t
                j_of[cy, cx] = j
                sy, scb, scr = self.palette[k]
                dd = pd(sy, t[0]) + (pd(scb, t[1]) + pd(scr, t[2]) if self.chroma else 0)
                dec[cy, cx] = (dd, c_y, c_c, m, F, cand, (0,) * 5)
        params = []
        for c in range(3 if self.chroma else 1):
            p = np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
            for cy in range(rows):
                for cx in range(cols):
                    p[cy, cx] = final[cy][cx][c]
            params.append(p)
        return {"params": params + [None] * (3 - len(params)), "decision": dec, "j": j_of, "j_new": j_new}

    def stats(self, idx):
        """the three statistics arrays of a grid: (rows, cols) of STATS_DTYPE each"""
        out = []
        for c in range(3):
            records = np.zeros(len(self.palette), S.STATS_DTYPE)
            for k, rec in enumerate(self.palette):
                records[k] = rec[c]
            out.append(records[idx])
        return out


# ---- palettes and grids ---------------------------------------------------------------------------------------------------------

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def record(rng, bit_depth, *, extreme=False):
    """one statistics record.  Ordinary: a few hundred samples per edge bin and in eight neighbouring bands, each bin with a mean
    error of its own inside +-(M + 1) -- the pick has something to choose in every bin.  extreme: counts and sums at the int32 ends"""
    st = np.zeros((), S.STATS_DTYPE)
    if extreme:
        st["eo_count"] = rng.choice([0, 1, 3, INT32_MAX], (4, 4))
        st["eo_sum"] = rng.choice([INT32_MIN, INT32_MAX, -1, 0], (4, 4))
        st["bo_count"] = rng.choice([0, 1, 2, INT32_MAX], 32)
        st["bo_sum"] = rng.choice([INT32_MIN, INT32_MAX, 1, 0], 32)
        return st
    M = S.max_offset(bit_depth)

    def bins(shape):
        n = rng.integers(0, 400, shape)
        return n, np.rint(n * rng.uniform(-M - 1, M + 1, shape)).astype(np.int64) + rng.integers(-3, 4, shape)
    st["eo_count"], st["eo_sum"] = bins((4, 4))
    st["eo_sum"][:, :2] = np.abs(st["eo_sum"][:, :2])           # valleys ask for positive offsets, peaks for negative ones
    st["eo_sum"][:, 2:] = -np.abs(st["eo_sum"][:, 2:])
    first = int(rng.integers(0, 32))
    n, s = bins(8)
    for j in range(8):
        st["bo_count"][(first + j) & 31], st["bo_sum"][(first + j) & 31] = n[j], s[j]
    return st


def nudged(st, rng):
    """a record close to st: every sum moved by a few per cent -- a neighbour's triple fits it nearly as well as its own"""
    out = st.copy()
    for f in ("eo_sum", "bo_sum"):
        out[f] = np.clip(np.rint(st[f] * rng.uniform(0.9, 1.1, st[f].shape)), INT32_MIN, INT32_MAX)
    return out


def palette(rng, bd_luma, bd_chroma, *, bases=6, variants=3, extreme=False):
    """bases * variants records (S_y, S_cb, S_cr): each base followed by its nudged variants"""
    out = []
    for _ in range(bases):
        base = [record(rng, bd, extreme=extreme) for bd in (bd_luma, bd_chroma, bd_chroma)]
        out.append(tuple(base))
        for _ in range(variants - 1):
            out.append(tuple(record(rng, bd, extreme=True) if extreme else nudged(b, rng) for b, bd in zip(base, (bd_luma, bd_chroma, bd_chroma))))
    return out


def grid_of(rows, cols, n_records, rng, *, variants=3, block=(3, 4)):
    """indices into a palette of n_records: blocks of block[0] x block[1] CTBs, each FLAT (one record: merges left), STRIPED (one
    record per column: merges up), MIXED (a record per CTB) or NEAR (variants of one base per CTB)"""
    idx = np.zeros((rows, cols), np.int64)
    per_col = rng.integers(0, n_records, cols)
    for by in range(0, rows, block[0]):
        for bx in range(0, cols, block[1]):
            kind = int(rng.integers(0, 4))
            sl = (slice(by, min(by + block[0], rows)), slice(bx, min(bx + block[1], cols)))
            shape = idx[sl].shape
            if kind == 0:
                idx[sl] = rng.integers(0, n_records)
            elif kind == 1:
                idx[sl] = np.broadcast_to(per_col[sl[1]], shape)
            elif kind == 2:
                idx[sl] = rng.integers(0, n_records, shape)
            else:
                idx[sl] = int(rng.integers(0, n_records // variants)) * variants + rng.integers(0, variants, shape)
    return idx


def banded(rows, cols, n_records, *, variants=3):
    """the same three behaviours for a grid too small for blocks, a third of the rows each: STRIPED rows (one record per column), FLAT
    rows (one record per row), then rows in which every CTB's left and upper neighbour come from another base"""
    idx = np.zeros((rows, cols), np.int64)
    bases = n_records // variants
    a, b = (rows + 2) // 3, (2 * rows + 2) // 3
    for cy in range(rows):
        for cx in range(cols):
            if cy < a:
                idx[cy, cx] = (cx * variants) % n_records
            elif cy < b:
                idx[cy, cx] = (cy * variants + 1) % n_records
            else:
                idx[cy, cx] = ((2 * cx + 3 * cy) % bases) * variants + 2
    return idx


def layout(rows, cols, kind):
    """(slice_idx, tile_idx) uint16 grids, or None: 'none'; 'slices' -- raster runs that end mid-row; 'tiles' -- 2 x 2 tiles (where the
    grid allows) in one slice; 'both'; 'ctb_slices' -- one CTB per slice"""
    if kind == "none":
        return None, None
    raster = np.arange(rows * cols).reshape(rows, cols)
    run = max(cols + cols // 2, 2)
    sl = (raster // run).astype(np.uint16)
    tl = ((np.arange(rows)[:, None] >= (rows + 1) // 2) * 2 + (np.arange(cols)[None, :] >= (cols + 1) // 2)).astype(np.uint16)
    if kind == "slices":
        return sl, None
    if kind == "tiles":
        return None, tl
    if kind == "both":
        return (tl * 8 + (raster // max(cols // 2, 1)) % 8).astype(np.uint16), tl   # slices inside tiles
    if kind == "ctb_slices":
        return raster.astype(np.uint16), None
    raise ValueError(kind)


def census(res):
    """what a decided grid exercises: the share of each `merge` among the CTBs with both candidates, the longest chain of
    merge-lefts, and whether a merge-up took its triple from a CTB that itself merged"""
    d = res["decision"]
    both = d["cand"] == 3
    share = [float((d["merge"][both] == m).mean()) if both.any() else 0.0 for m in range(3)]
    chain = best = 0
    for row in d["merge"]:
        chain = 0
        for m in row:
            chain = chain + 1 if m == 1 else 0
            best = max(best, chain)
    up_of_merged = bool(((d["merge"][1:] == 2) & (d["merge"][:-1] != 0)).any())
    return {"share": share, "left_chain": best, "up_of_merged": up_of_merged}


GRIDS = ((1, 1), (1, 9), (9, 1), (5, 7), (61, 34))   # columns x rows, as the issue names them
