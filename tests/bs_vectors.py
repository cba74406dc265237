"""Boundary strength derivation (H.265 8.7.2.4): a second reference written as a statement about sets, and the vectors.

TEST INFRASTRUCTURE ONLY.  oracle/h265_oracle.c::bs_of_edge and csrc/deblock_h265.h::h265_bs_of_edge are one decision tree
written twice; this module states the rule in another shape so that agreement means something:

* an edge segment EXISTS iff the Q unit flags a transform or prediction edge in that direction, the segment lies on the
  8x8 luma grid strictly inside the picture, and Q carries neither DBK_OFF nor the direction's NOX flag;
* bS 2 iff either side is intra; else bS 1 iff it is a TRANSFORM edge and either side has CBF;
* else let M(P), M(Q) be the multisets of (reference picture, mv) the sides use (0, 1 or 2 entries, list membership
  forgotten): bS 0 iff |M(P)| = |M(Q)| and some one-to-one pairing of M(P) with M(Q) pairs equal pictures whose vectors
  differ by less than 4 (quarter samples) in both components; bS 1 otherwise;
* KEEP_P / KEEP_Q are attached iff bS > 0.

segment_bs() is that text in plain Python ints (itertools.permutations over the entries a side uses); derive_bs() is the
same statement over whole pictures in numpy int64 (a pairing = a permutation of the two list slots under which every slot
is either used on both sides and matching, or unused on both sides), which no int16 / int32 operand can overflow.  The
CPU tests tie the two together segment by segment.

Decisions taken where the rule's wording leaves room (the H.265 text is not available to this project; the sources are
include/hevc_deblock.h, DESIGN.md 4.4 and the hand-worked cases of test_h265_oracle.py::test_bs_rules):
  - the switches (DBK_OFF, NOX) and the edge flags are read from the Q unit only: the edge belongs to the block whose
    left / top border it is.  The same bits on the P unit change nothing.
  - CBF counts on a transform edge only; on a prediction-only edge the motion rule decides even when both sides have CBF.
  - two inter units that both use no list (count 0 = count 0, empty pairing) give bS 0.
  - the unused list slots of a unit are never read, whatever they hold.
No disagreement between this reference and the oracle was found (see tests/test_bs_rules_cpu.py).

chroma_bs() restates "the luma entry at bS[xDk * SubWidthC][yDm * SubHeightC]" in sample coordinates for
chroma_format_idc 1, 2, 3, independent of rext_oracle.chroma_bs and oracle.h265.chroma_bs.

Generators (seeded, integer only): rule_product, extreme_cases, coded_picture; census() reports which leaf of the rule each
segment reached, with which result, and for every vector comparison that decided a result its signed difference.
"""
import itertools
from collections import Counter

import numpy as np

BS_MASK, KEEP_P, KEEP_Q = 3, 4, 8
U_INTRA, U_CBF, U_TU_LEFT, U_TU_TOP, U_PU_LEFT, U_PU_TOP = 1, 2, 4, 8, 16, 32
U_KEEP, U_DBK_OFF, U_PRED_L0, U_PRED_L1, U_NOX_LEFT, U_NOX_TOP = 64, 128, 256, 512, 1024, 2048
UNIT_DTYPES = (np.uint16, np.int16, np.int16, np.int32, np.int32)
SUB = {1: (2, 2), 2: (2, 1), 3: (1, 1)}  # chroma_format_idc -> (SubWidthC, SubHeightC)
INT16_MIN, INT16_MAX, INT32_MIN, INT32_MAX = -32768, 32767, -2 ** 31, 2 ** 31 - 1

LEAVES = ("no_edge", "dbk_off", "nox", "intra", "cbf", "count_differs", "no_motion", "pictures_differ", "one_vector",
          "two_pictures_straight", "two_pictures_crossed", "one_picture")
# the results a leaf can give
LEAF_RESULTS = {"no_edge": (0,), "dbk_off": (0,), "nox": (0,), "intra": (2,), "cbf": (1,), "count_differs": (1,),
                "no_motion": (0,), "pictures_differ": (1,), "one_vector": (0, 1), "two_pictures_straight": (0, 1),
                "two_pictures_crossed": (0, 1), "one_picture": (0, 1)}
# the (P list, Q list) comparisons that can decide each vector leaf
LEAF_COMPARISONS = {"one_vector": ((0, 0), (0, 1), (1, 0), (1, 1)), "two_pictures_straight": ((0, 0), (1, 1)),
                    "two_pictures_crossed": ((0, 1), (1, 0)), "one_picture": ((0, 0), (0, 1), (1, 0), (1, 1))}
# each component at -4, -3, +3, +4 while the other is 0 and while it is +-3
THRESHOLD_DIFFS = tuple(sorted({(a, b) for a in (-4, -3, 3, 4) for b in (0, -3, 3)} | {(b, a) for a in (-4, -3, 3, 4) for b in (0, -3, 3)}))


def _dir_bits(left):
    return (U_TU_LEFT, U_PU_LEFT, U_NOX_LEFT) if left else (U_TU_TOP, U_PU_TOP, U_NOX_TOP)


# ---- the reference, one segment at a time, Python ints ---------------------------------------------------------------

def motion_multiset(flags, mv0, mv1, ref0, ref1):
    """the (picture, mvx, mvy) entries a unit uses, list membership forgotten"""
    m = []
    if flags & U_PRED_L0:
        m.append((int(ref0), int(mv0[0]), int(mv0[1])))
    if flags & U_PRED_L1:
        m.append((int(ref1), int(mv1[0]), int(mv1[1])))
    return m


def segment_bs(fp, fq, mp, mq, left):
    """the bS entry of a segment on the grid inside the picture; fp / fq = flags of the P / Q unit, mp / mq = motion_multiset"""
    tu, pu, nox = _dir_bits(left)
    if not fq & (tu | pu) or fq & (U_DBK_OFF | nox):
        return 0
    if (fp | fq) & U_INTRA:
        bs = 2
    elif fq & tu and (fp | fq) & U_CBF:
        bs = 1
    else:
        same = len(mp) == len(mq) and any(
            all(a[0] == b[0] and abs(a[1] - b[1]) < 4 and abs(a[2] - b[2]) < 4 for a, b in zip(mp, perm))
            for perm in itertools.permutations(mq))
        bs = 0 if same else 1
    if bs == 0:
        return 0
    return bs | (KEEP_P if fp & U_KEEP else 0) | (KEEP_Q if fq & U_KEEP else 0)


def derive_bs_scalar(units, w, h):
    """segment_bs over every segment of a w x h picture; (vert, hor) in the library's layout"""
    f, mv0, mv1, r0, r1 = (np.asarray(a).tolist() for a in units)
    uw, uh = w // 4, h // 4
    vert = np.zeros((uh, w // 8 + 1), np.uint8)
    hor = np.zeros((h // 8 + 1, uw), np.uint8)

    def ms(y, x):
        return motion_multiset(f[y][x], mv0[y][x], mv1[y][x], r0[y][x], r1[y][x])

    for y4 in range(uh):
        for bx in range(1, w // 8):
            vert[y4, bx] = segment_bs(f[y4][2 * bx - 1], f[y4][2 * bx], ms(y4, 2 * bx - 1), ms(y4, 2 * bx), True)
    for by in range(1, h // 8):
        for x4 in range(uw):
            hor[by, x4] = segment_bs(f[2 * by - 1][x4], f[2 * by][x4], ms(2 * by - 1, x4), ms(2 * by, x4), False)
    return vert.ravel(), hor.ravel()


# ---- the reference over whole pictures, numpy int64 ------------------------------------------------------------------

class _Sides:
    """the P and Q units of every interior segment of one direction, as int64"""

    def __init__(self, units, w, h, left):
        f, mv0, mv1, r0, r1 = units
        uw, uh = w // 4, h // 4
        if left:
            p, q = (slice(None), slice(1, max(uw - 1, 1), 2)), (slice(None), slice(2, uw, 2))
        else:
            p, q = (slice(1, max(uh - 1, 1), 2), slice(None)), (slice(2, uh, 2), slice(None))
        g = lambda a, s: np.asarray(a)[s].astype(np.int64)
        self.fp, self.fq = g(f, p), g(f, q)
        self.pref, self.qref = (g(r0, p), g(r1, p)), (g(r0, q), g(r1, q))
        self.pmv, self.qmv = (g(mv0, p), g(mv1, p)), (g(mv0, q), g(mv1, q))
        self.left = left


class _Rule:
    def __init__(self, s):
        tu, pu, nox = _dir_bits(s.left)
        fp, fq = s.fp, s.fq
        self.flagged = (fq & (tu | pu)) != 0
        self.off = (fq & U_DBK_OFF) != 0
        self.nox = (fq & nox) != 0
        self.exists = self.flagged & ~self.off & ~self.nox
        self.intra = ((fp | fq) & U_INTRA) != 0
        self.coded = ((fq & tu) != 0) & (((fp | fq) & U_CBF) != 0)
        self.up = [(fp & U_PRED_L0) != 0, (fp & U_PRED_L1) != 0]
        self.uq = [(fq & U_PRED_L0) != 0, (fq & U_PRED_L1) != 0]
        self.same = [[s.pref[i] == s.qref[j] for j in (0, 1)] for i in (0, 1)]
        self.diff = [[s.pmv[i] - s.qmv[j] for j in (0, 1)] for i in (0, 1)]
        self.near = [[(np.abs(self.diff[i][j]) < 4).all(axis=-1) for j in (0, 1)] for i in (0, 1)]
        self.paired = self.pairing_exists(self.near)
        bs = np.where(~self.exists, 0, np.where(self.intra, 2, np.where(self.coded, 1, np.where(self.paired, 0, 1))))
        keep = np.where((fp & U_KEEP) != 0, KEEP_P, 0) | np.where((fq & U_KEEP) != 0, KEEP_Q, 0)
        self.bs = bs
        self.entry = np.where(bs > 0, bs | keep, 0).astype(np.uint8)

    def pairing_exists(self, near):
        """some permutation of the two list slots under which every slot is used on both sides by equal pictures with near
        vectors, or used on neither side"""
        out = np.zeros(self.exists.shape, bool)
        for perm in ((0, 1), (1, 0)):
            ok = np.ones(self.exists.shape, bool)
            for i in (0, 1):
                j = perm[i]
                ok &= (self.up[i] & self.uq[j] & self.same[i][j] & near[i][j]) | (~self.up[i] & ~self.uq[j])
            out |= ok
        return out


def derive_bs(units, w, h):
    """8.7.2.4 for a w x h picture: (vert, hor) uint8 in the library's layout; picture-boundary entries are 0"""
    vert = np.zeros((h // 4, w // 8 + 1), np.uint8)
    hor = np.zeros((h // 8 + 1, w // 4), np.uint8)
    if w >= 16:
        vert[:, 1:w // 8] = _Rule(_Sides(units, w, h, True)).entry
    if h >= 16:
        hor[1:h // 8, :] = _Rule(_Sides(units, w, h, False)).entry
    return vert.ravel(), hor.ravel()


def chroma_bs(vert, hor, w, h, chroma_format_idc):
    """the bS arrays of the (w / SubWidthC) x (h / SubHeightC) chroma plane: the entry of the chroma edge segment that starts
    at chroma sample (xDk, yDm) is the luma entry of the segment holding luma sample (xDk * SubWidthC, yDm * SubHeightC)"""
    sx, sy = SUB[chroma_format_idc]
    cw, ch = w // sx, h // sy
    lv = np.asarray(vert, np.uint8).reshape(h // 4, w // 8 + 1)
    lh = np.asarray(hor, np.uint8).reshape(h // 8 + 1, w // 4)
    cv = np.zeros((ch // 4, cw // 8 + 1), np.uint8)
    chh = np.zeros((ch // 8 + 1, cw // 4), np.uint8)
    # vertical chroma edges: xDk = 8 * k, segments start at yDm = 4 * m
    for k in range(cw // 8 + 1):
        lx = 8 * k * sx
        ly = 4 * np.arange(ch // 4) * sy
        cv[:, k] = lv[ly // 4, lx // 8]
    # horizontal chroma edges: yDm = 8 * k, segments start at xDk = 4 * m
    for k in range(ch // 8 + 1):
        ly = 8 * k * sy
        lx = 4 * np.arange(cw // 4) * sx
        chh[k, :] = lh[ly // 8, lx // 4]
    return cv.ravel(), chh.ravel()


# ---- census ----------------------------------------------------------------------------------------------------------

def _empty_census():
    return {d: {"leaf": {l: Counter() for l in LEAVES}, "keep": Counter(), "off_grid": 0, "boundary": 0,
                "diff": {(l, c): Counter() for l in LEAF_COMPARISONS for c in LEAF_COMPARISONS[l]}} for d in ("vert", "hor")}


def merge_census(a, b):
    for d in a:
        for l in LEAVES:
            a[d]["leaf"][l].update(b[d]["leaf"][l])
        a[d]["keep"].update(b[d]["keep"])
        a[d]["off_grid"] += b[d]["off_grid"]
        a[d]["boundary"] += b[d]["boundary"]
        for k in a[d]["diff"]:
            a[d]["diff"][k].update(b[d]["diff"][k])
    return a


def _count_rows(rows):
    if not len(rows):
        return Counter()
    vals, n = np.unique(rows, axis=0, return_counts=True)
    return Counter({tuple(int(x) for x in v): int(c) for v, c in zip(vals, n)})


def census(units, w, h):
    """Per direction ("vert" / "hor"): "leaf"[name] = Counter {bS: segments} of the interior on-grid segments that ended in
    that leaf of the rule; "keep" = Counter {(bS, keep P, keep Q)}; "off_grid" / "boundary" = units flagging an edge of
    that direction off the 8x8 grid / on the picture boundary (no entry exists for them); "diff"[(leaf, (P list, Q list))] =
    Counter {(dx, dy)} of P's minus Q's vector for the comparisons that DECIDED the result: between equal pictures, and the
    result would be the other one had this comparison come out the other way."""
    out = _empty_census()
    flags = np.asarray(units[0]).astype(np.int64)
    for left, name in ((True, "vert"), (False, "hor")):
        c = out[name]
        tu, pu, _ = _dir_bits(left)
        fl = (flags & (tu | pu)) != 0
        c["off_grid"] = int(fl[:, 1::2].sum() if left else fl[1::2, :].sum())
        c["boundary"] = int(fl[:, 0].sum() if left else fl[0, :].sum())
        if (w if left else h) < 16:
            continue
        s = _Sides(units, w, h, left)
        r = _Rule(s)
        n_p, n_q = r.up[0].astype(int) + r.up[1], r.uq[0].astype(int) + r.uq[1]
        motion = r.exists & ~r.intra & ~r.coded
        pics1 = np.zeros(r.exists.shape, bool)
        for i in (0, 1):
            for j in (0, 1):
                pics1 |= r.up[i] & r.uq[j] & r.same[i][j]
        straight, crossed = r.same[0][0] & r.same[1][1], r.same[0][1] & r.same[1][0]
        two = motion & (n_p == 2) & (n_q == 2)
        one_pic = s.pref[0] == s.pref[1]
        masks = {
            "no_edge": ~r.flagged, "dbk_off": r.flagged & r.off, "nox": r.flagged & ~r.off & r.nox,
            "intra": r.exists & r.intra, "cbf": r.exists & ~r.intra & r.coded,
            "count_differs": motion & (n_p != n_q), "no_motion": motion & (n_p == 0) & (n_q == 0),
            "pictures_differ": (motion & (n_p == 1) & (n_q == 1) & ~pics1) | (two & ~straight & ~crossed),
            "one_vector": motion & (n_p == 1) & (n_q == 1) & pics1,
            "two_pictures_straight": two & straight & ~one_pic, "two_pictures_crossed": two & crossed & ~straight & ~one_pic,
            "one_picture": two & straight & one_pic}
        total = np.zeros(r.exists.shape, int)
        for leaf, m in masks.items():
            total += m
            c["leaf"][leaf].update(Counter(int(x) for x in r.bs[m]))
        assert (total == 1).all()  # the leaves partition the segments
        kp, kq = (r.entry & KEEP_P) != 0, (r.entry & KEEP_Q) != 0
        c["keep"] = _count_rows(np.stack([r.bs.ravel(), kp.ravel(), kq.ravel()], axis=1))
        for (leaf, (i, j)) in c["diff"]:
            near = [[r.near[a][b] for b in (0, 1)] for a in (0, 1)]
            near[i][j] = ~near[i][j]
            decides = masks[leaf] & r.up[i] & r.uq[j] & r.same[i][j] & (r.pairing_exists(near) != r.paired)
            c["diff"][(leaf, (i, j))] = _count_rows(r.diff[i][j][decides])
    return out


# ---- cases: one edge segment each, packed into pictures --------------------------------------------------------------

KINDS = ("intra", "inter_no_motion", "l0", "l1", "both")
_KIND_FLAGS = np.array([U_INTRA, 0, U_PRED_L0, U_PRED_L1, U_PRED_L0 | U_PRED_L1], np.int64)


class Cases:
    """n edge segments.  Per side s in "pq": base[s] = the direction-free flags (INTRA, CBF, KEEP, DBK_OFF, PRED_L0/1),
    tu[s] / pu[s] / nox[s] = the edge and NOX flag of the direction the cases get packed along, mv[s][l] (n, 2) and ref[s][l]
    (n,) = list l's slot, all int64."""

    def __init__(self, n):
        self.n = n
        z = lambda *shape: np.zeros((n,) + shape, np.int64)
        self.base = {s: z() for s in "pq"}
        self.tu, self.pu, self.nox = ({s: z() for s in "pq"} for _ in range(3))
        self.mv = {s: [z(2), z(2)] for s in "pq"}
        self.ref = {s: [z(), z()] for s in "pq"}

    @staticmethod
    def concat(parts):
        out = Cases(sum(p.n for p in parts))
        for s in "pq":
            for name in ("base", "tu", "pu", "nox"):
                getattr(out, name)[s] = np.concatenate([getattr(p, name)[s] for p in parts])
            for l in (0, 1):
                out.mv[s][l] = np.concatenate([p.mv[s][l] for p in parts])
                out.ref[s][l] = np.concatenate([p.ref[s][l] for p in parts])
        return out

    def set_kinds(self, pk, qk):
        self.base["p"] |= _KIND_FLAGS[pk]
        self.base["q"] |= _KIND_FLAGS[qk]

    def used(self, s, l):
        return (self.base[s] & (U_PRED_L0, U_PRED_L1)[l]) != 0

    def poison_unused(self, rng, refs):
        """every slot a unit does not use (both lists of intra units and of inter units without motion, the other list of
        uni-predicted ones) gets values that flip the result of a rule that reads it: the other side's entry (a false match)
        or a far vector / another picture (a false difference), chosen by the generator"""
        for s, o in ("pq", "qp"):
            for l in (0, 1):
                free = ~self.used(s, l)
                pick = rng.integers(0, 4, self.n)
                # the other side's slot that IS used (list l if it is, else the other list)
                o_l = np.where(self.used(o, l), l, 1 - l)
                o_mv = np.where((o_l == 0)[:, None], self.mv[o][0], self.mv[o][1])
                o_ref = np.where(o_l == 0, self.ref[o][0], self.ref[o][1])
                far = np.clip(o_mv + rng.choice(np.array([-9, -4, 4, 9]), (self.n, 2)), INT16_MIN, INT16_MAX)
                other_pic = np.where(o_ref == refs[0], refs[1], refs[0])
                mv = np.where((pick == 0)[:, None], o_mv, np.where((pick == 1)[:, None], far, rng.integers(INT16_MIN, INT16_MAX + 1, (self.n, 2))))
                ref = np.where(pick == 0, o_ref, np.where(pick == 1, o_ref, other_pic))
                self.mv[s][l] = np.where(free[:, None], mv, self.mv[s][l])
                self.ref[s][l] = np.where(free, ref, self.ref[s][l])


def pack_cases(cases, left, nb, seed):
    """One picture whose interior segments of one direction are the cases: with left, case k sits at 8-sample column
    bx = 1 + k % nb of unit row k // nb and owns units 2 * bx - 1 (P) and 2 * bx (Q); without, the picture is the same thing
    along horizontal edges (case k at 8-sample row by = 1 + k % nb, unit column k // nb).  Flags of the OTHER direction are
    sprinkled in by the generator so that the picture's other array is not empty.  Returns (units, w, h)."""
    rng = np.random.default_rng(seed)
    rows = -(-cases.n // nb)
    rows += (-rows) % 4                      # 4 unit rows = 16 samples: every chroma format's entry takes the picture
    across = 2 * (nb + 1)                    # units across the edges; nb + 1 even -> a multiple of 16 samples
    assert (nb + 1) % 2 == 0
    tu, pu, nox = _dir_bits(left)
    otu, opu, onox = _dir_bits(not left)
    flags = np.zeros((rows, across), np.int64)
    mv = [np.zeros((rows, across, 2), np.int64) for _ in (0, 1)]
    ref = [np.zeros((rows, across), np.int64) for _ in (0, 1)]
    k = np.arange(cases.n)
    r, b = k // nb, 1 + k % nb
    for s, col in (("p", 2 * b - 1), ("q", 2 * b)):
        flags[r, col] = cases.base[s] | cases.tu[s] * tu | cases.pu[s] * pu | cases.nox[s] * nox
        for l in (0, 1):
            mv[l][r, col] = cases.mv[s][l]
            ref[l][r, col] = cases.ref[s][l]
    other = rng.integers(0, 16, flags.shape)
    flags |= np.where(other == 0, otu, 0) | np.where(other == 1, opu, 0) | np.where(other == 2, otu | opu, 0) | \
        np.where(other == 3, otu | onox, 0)
    units = [flags, mv[0], mv[1], ref[0], ref[1]]
    if not left:
        units = [np.swapaxes(a, 0, 1) for a in units]
    units = tuple(np.ascontiguousarray(a).astype(dt) for a, dt in zip(units, UNIT_DTYPES))
    uh, uw = units[0].shape
    return units, 4 * uw, 4 * uh


def _entries_to_slots(c, s, kind, ea, eb, crossed):
    """side s of kind `kind` (KINDS index per case) holding the entries ea (and eb when it uses both lists): list 0 = ea,
    list 1 = eb, or the other way round where crossed; a side that uses one list holds ea in it"""
    (ra, ma), (rb, mb) = ea, eb
    both = kind == 4
    first_b = both & crossed
    c.ref[s][0] = np.where(first_b, rb, ra)
    c.mv[s][0] = np.where(first_b[:, None], mb, ma)
    c.ref[s][1] = np.where(both & ~crossed, rb, ra)
    c.mv[s][1] = np.where((both & ~crossed)[:, None], mb, ma)


PICTURES = (-1, 0, 5)      # the three-picture alphabet (POCs; negative ones occur in real streams)
DELTAS = (0, -3, 3, -4, 4)


def _grid(*axes):
    return np.array(list(itertools.product(*axes)), np.int64).reshape(-1, len(axes))


def _flag_cases(rng):
    """side kind x CBF x KEEP for each side; Q's edge kind {none, TU, PU, TU+PU} x DBK_OFF x NOX; DBK_OFF, NOX and edge flags
    on the P unit as distractors; the motion of inter pairs drawn by the generator (equal, at the threshold, another picture,
    crossed)"""
    g = _grid(range(5), (0, 1), (0, 1), range(5), (0, 1), (0, 1), range(4), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1))
    c = Cases(len(g))
    pk, pcbf, pkeep, qk, qcbf, qkeep, edge, off, nox, p_off, p_nox, p_edge = g.T
    c.set_kinds(pk, qk)
    c.base["p"] |= pcbf * U_CBF | pkeep * U_KEEP | p_off * U_DBK_OFF
    c.base["q"] |= qcbf * U_CBF | qkeep * U_KEEP | off * U_DBK_OFF
    c.tu["q"], c.pu["q"], c.nox["q"] = edge & 1, edge >> 1, nox
    c.tu["p"], c.pu["p"], c.nox["p"] = p_edge, p_edge, p_nox
    n = c.n
    pics = np.array(PICTURES)
    ea = (pics[rng.integers(0, 3, n)], rng.integers(-100, 101, (n, 2)))
    eb = (pics[rng.integers(0, 3, n)], rng.integers(-100, 101, (n, 2)) + 400)
    var = rng.integers(0, 4, n)   # 0 equal, 1 one component at the threshold, 2 another picture, 3 within the threshold
    step = np.zeros((n, 2), np.int64)
    step[np.arange(n), rng.integers(0, 2, n)] = np.where(var == 1, 4, np.where(var == 3, 3, 0)) * rng.choice(np.array([-1, 1]), n)
    qa = (np.where(var == 2, pics[(np.searchsorted(pics, ea[0]) + 1) % 3], ea[0]), ea[1] + step)
    _entries_to_slots(c, "p", pk, ea, eb, np.zeros(n, bool))
    _entries_to_slots(c, "q", qk, qa, eb, rng.integers(0, 2, n) == 1)
    return c


def _one_vector_cases(rng, reps=4):
    """P and Q use one list each: which lists x the pictures x Q's vector = P's plus a delta from {0, +-3, +-4}^2"""
    g = _grid(range(reps), (2, 3), (2, 3), range(3), range(3), DELTAS, DELTAS)
    c = Cases(len(g))
    _, pk, qk, pr, qr, dx, dy = g.T
    c.set_kinds(pk, qk)
    pics = np.array(PICTURES)
    base = rng.integers(-2000, 2001, (c.n, 2))
    _entries_to_slots(c, "p", pk, (pics[pr], base), (pics[pr], base), np.zeros(c.n, bool))
    _entries_to_slots(c, "q", qk, (pics[qr], base + np.stack([dx, dy], 1)), (pics[qr], base), np.zeros(c.n, bool))
    return c


def _two_vector_cases(rng, sample=None):
    """P and Q use both lists: a picture from the alphabet in each of the four slots x Q's vectors = P's straight or crossed
    plus a delta per vector from {0, +-3, +-4}^2 (P's two vectors far apart); and, for one picture in all four slots, P's two
    vectors near each other (so that both pairings matter at once).  sample: keep that many of the cases, drawn by the
    generator (None: the full product)."""
    g = _grid(range(3), range(3), range(3), range(3), (0, 1), DELTAS, DELTAS, DELTAS, DELTAS)
    gaps = np.array([(0, 0), (3, 3), (4, 0), (0, -4), (7, -2)], np.int64)
    g2 = _grid(range(3), range(len(gaps)), DELTAS, DELTAS, DELTAS, DELTAS)
    if sample is not None:
        g = g[np.sort(rng.choice(len(g), min(sample, len(g)), replace=False))]
    n1, n2 = len(g), len(g2)
    c = Cases(n1 + n2)
    both = np.full(c.n, 4)
    c.set_kinds(both, both)
    pics = np.array(PICTURES)
    m0 = rng.integers(-2000, 2001, (c.n, 2))
    gap = np.concatenate([rng.choice(np.array([-1, 1]), (n1, 2)) * rng.integers(16, 200, (n1, 2)), gaps[g2[:, 1]]])
    m1 = m0 + gap
    crossed = np.concatenate([g[:, 4] == 1, np.zeros(n2, bool)])
    d0 = np.concatenate([g[:, 5:7], g2[:, 2:4]])
    d1 = np.concatenate([g[:, 7:9], g2[:, 4:6]])
    for l, r in ((0, np.concatenate([g[:, 0], g2[:, 0]])), (1, np.concatenate([g[:, 1], g2[:, 0]]))):
        c.ref["p"][l] = pics[r]
    for l, r in ((0, np.concatenate([g[:, 2], g2[:, 0]])), (1, np.concatenate([g[:, 3], g2[:, 0]]))):
        c.ref["q"][l] = pics[r]
    c.mv["p"][0], c.mv["p"][1] = m0, m1
    c.mv["q"][0] = np.where(crossed[:, None], m1, m0) + d0
    c.mv["q"][1] = np.where(crossed[:, None], m0, m1) + d1
    return c


def _motion_edges(c, rng):
    """the edge of a case whose motion is to decide: a prediction edge, a transform edge without coefficients, or both"""
    e = rng.integers(1, 4, c.n)
    c.tu["q"], c.pu["q"] = e & 1, e >> 1


def rule_product(seed=1, two_vector_sample=None, nb=255):
    """[(units, w, h) packed along vertical edges, (units, w, h) packed along horizontal edges] of the product of the rule's
    inputs, one case per edge segment"""
    rng = np.random.default_rng(seed)
    flag = _flag_cases(rng)
    one, two = _one_vector_cases(rng), _two_vector_cases(rng, two_vector_sample)
    _motion_edges(one, rng)
    _motion_edges(two, rng)
    cases = Cases.concat([flag, one, two])
    cases.poison_unused(rng, PICTURES)
    return [pack_cases(cases, True, nb, seed + 1), pack_cases(cases, False, nb, seed + 2)]


# component pairs (P's, Q's) at the int16 ends: true differences 0, 3, 4 (decided correctly by 16-bit arithmetic as well) and
# 65533, 65535 (which wrap to 3 and 1 in 16 bits: a narrowed subtraction calls them near)
_END_PAIRS = ((-32768, -32768), (32767, 32767), (-32768, -32765), (32764, 32767), (-32768, -32764), (32763, 32767),
              (-32766, 32767), (-32768, 32767), (-32765, -32768), (32767, 32764), (-32764, -32768), (32767, 32763),
              (32767, -32766), (32767, -32768))
_END_NEAR = ((-32768, -32768), (32767, 32767), (-32768, -32765), (32767, 32764), (32764, 32764), (-32765, -32765))
END_PICTURES = (INT32_MIN, -1, 0, 1, INT32_MAX)


def extreme_cases(seed=2, nb=63):
    """the rules at the ends of the operand ranges, packed like rule_product: vector components from {-32768, -32766, -32765,
    -32764, 32763, 32764, 32767} paired so that true differences are 0, 3, 4, 65533 and 65535; pictures from {INT32_MIN,
    -1, 0, 1, INT32_MAX} (equal ones held in different lists, unequal ones whose 32-bit difference wraps); unused slots
    poisoned"""
    rng = np.random.default_rng(seed)
    pics = np.array(END_PICTURES)
    ends, nears = np.array(_END_PAIRS, np.int64), np.array(_END_NEAR, np.int64)
    parts = []
    # one vector a side: the deciding component takes every end pair, the other one a near pair; x and y in turn
    g = _grid((2, 3), (2, 3), range(5), range(len(ends)), range(len(nears)), (0, 1))
    c = Cases(len(g))
    pk, qk, r, e, m, comp = g.T
    c.set_kinds(pk, qk)
    pv = np.where((comp == 0)[:, None], np.stack([ends[e, 0], nears[m, 0]], 1), np.stack([nears[m, 0], ends[e, 0]], 1))
    qv = np.where((comp == 0)[:, None], np.stack([ends[e, 1], nears[m, 1]], 1), np.stack([nears[m, 1], ends[e, 1]], 1))
    no = np.zeros(c.n, bool)
    _entries_to_slots(c, "p", pk, (pics[r], pv), (pics[r], pv), no)
    _entries_to_slots(c, "q", qk, (pics[r], qv), (pics[r], qv), no)
    parts.append(c)
    # one vector a side, equal vectors at an end, every ordered pair of pictures
    g = _grid((2, 3), (2, 3), range(5), range(5), range(len(nears)))
    c = Cases(len(g))
    pk, qk, pr, qr, m = g.T
    c.set_kinds(pk, qk)
    no = np.zeros(c.n, bool)
    pv, qv = np.stack([nears[m, 0], nears[m, 0]], 1), np.stack([nears[m, 1], nears[m, 1]], 1)
    _entries_to_slots(c, "p", pk, (pics[pr], pv), (pics[pr], pv), no)
    _entries_to_slots(c, "q", qk, (pics[qr], qv), (pics[qr], qv), no)
    parts.append(c)
    # two vectors a side: pictures (ra, rb) on P, the same two on Q straight or crossed; entry a's deciding component takes
    # every end pair while entry b is near, and the other way round
    g = _grid(range(5), range(5), (0, 1), range(len(ends)), range(len(nears)), (0, 1), (0, 1))
    c = Cases(len(g))
    ra, rb, cr, e, m, comp, which = g.T
    both = np.full(c.n, 4)
    c.set_kinds(both, both)
    dec_p = np.where((comp == 0)[:, None], np.stack([ends[e, 0], nears[m, 0]], 1), np.stack([nears[m, 0], ends[e, 0]], 1))
    dec_q = np.where((comp == 0)[:, None], np.stack([ends[e, 1], nears[m, 1]], 1), np.stack([nears[m, 1], ends[e, 1]], 1))
    oth_p = np.stack([nears[m, 1], nears[(m + 1) % len(nears), 0]], 1)
    oth_q = np.stack([nears[m, 1], nears[(m + 1) % len(nears), 1]], 1)
    w0 = (which == 0)[:, None]
    pa, pb = np.where(w0, dec_p, oth_p), np.where(w0, oth_p, dec_p)
    qa, qb = np.where(w0, dec_q, oth_q), np.where(w0, oth_q, dec_q)
    _entries_to_slots(c, "p", both, (pics[ra], pa), (pics[rb], pb), np.zeros(c.n, bool))
    _entries_to_slots(c, "q", both, (pics[ra], qa), (pics[rb], qb), cr == 1)
    parts.append(c)
    # two vectors a side with pictures that differ in one slot only, at the ends of int32
    g = _grid(range(5), range(5), range(5), (0, 1), range(len(nears)))
    c = Cases(len(g))
    ra, rb, rc, cr, m = g.T
    both = np.full(c.n, 4)
    c.set_kinds(both, both)
    v = np.stack([nears[m, 0], nears[m, 0]], 1)
    _entries_to_slots(c, "p", both, (pics[ra], v), (pics[rb], v), np.zeros(c.n, bool))
    _entries_to_slots(c, "q", both, (pics[ra], v), (pics[rc], v), cr == 1)
    parts.append(c)
    for c in parts:
        _motion_edges(c, rng)
    # intra and motion-less units whose slots hold the extremes; counts that differ
    g = _grid(range(5), range(5), range(len(ends)), range(5), (1, 2, 3))
    c = Cases(len(g))
    pk, qk, e, r, edge = g.T
    c.set_kinds(pk, qk)
    c.tu["q"], c.pu["q"] = edge & 1, edge >> 1
    for s, col in (("p", 0), ("q", 1)):
        for l in (0, 1):
            c.mv[s][l] = np.stack([ends[e, col], ends[(e + l) % len(ends), col]], 1)
            c.ref[s][l] = pics[(r + l * (s == "q")) % 5]
    parts.append(c)
    cases = Cases.concat(parts)
    cases.poison_unused(rng, (INT32_MIN, INT32_MAX))
    return [pack_cases(cases, True, nb, seed + 1), pack_cases(cases, False, nb, seed + 2)]


# ---- decoder-shaped pictures -----------------------------------------------------------------------------------------

def coded_picture(w, h, seed, ctb_log2=6):
    """Units as a decoder produces them for a w x h picture (multiples of 8): CTBs of 1 << ctb_log2 (16 / 32 / 64), a coding
    quadtree down to 8x8 (forced at the picture's right and bottom border), prediction partitions 2Nx2N / 2NxN / Nx2N / NxN
    and the four asymmetric ones, transform trees down to 4x4, merge-like motion copied from the left or upper neighbour
    (with and without a small refinement), slices as runs of CTBs and tiles as a grid, both with NOX on their borders
    where in-loop filtering must not cross, DBK_OFF per slice, PCM / bypass blocks with KEEP.  Edge flags sit on the first
    row / column of units of a block only; motion is constant inside a prediction block; the slots a block does not use
    hold whatever the generator left there."""
    assert w % 8 == 0 and h % 8 == 0 and ctb_log2 in (4, 5, 6)
    rng = np.random.default_rng(seed)
    uw, uh = w // 4, h // 4
    flags = np.zeros((uh, uw), np.int64)
    mv = [rng.integers(INT16_MIN, INT16_MAX + 1, (uh, uw, 2)) for _ in (0, 1)]
    ref = [rng.integers(-40, 40, (uh, uw)) for _ in (0, 1)]
    pocs = np.array([-16, -8, -4, -2, -1, 0, 1, 3, 8])
    cs = 1 << (ctb_log2 - 2)                       # CTB size in units
    cw, chh = -(-uw // cs), -(-uh // cs)
    # slices: runs of CTBs in raster order; tiles: a grid
    n_ctb = cw * chh
    slice_of = np.zeros(n_ctb, np.int64)
    starts = np.unique(rng.integers(0, n_ctb, max(1, n_ctb // 6)))
    slice_of[starts] = 1
    slice_of = np.cumsum(slice_of).reshape(chh, cw)
    n_slices = int(slice_of.max()) + 1
    slice_off = rng.integers(0, 5, n_slices) == 0          # slice_deblocking_filter_disabled_flag
    slice_nox = rng.integers(0, 2, n_slices) == 0          # slice_loop_filter_across_slices_enabled_flag == 0
    tile_cols = set(int(x) for x in rng.integers(1, max(cw, 2), 2)) if cw > 2 else set()
    tile_rows = set(int(x) for x in rng.integers(1, max(chh, 2), 1)) if chh > 2 else set()
    tiles_nox = bool(rng.integers(0, 2))

    def rect(a, x, y, bw, bh, v):
        a[y:y + bh, x:x + bw] = v

    def pred_block(x, y, bw, bh, intra):
        flags[y:y + bh, x] |= U_PU_LEFT
        flags[y, x:x + bw] |= U_PU_TOP
        if intra:
            return
        r = rng.integers(0, 10)
        src = None
        if r < 4 and x > 0 and not flags[y, x - 1] & U_INTRA:
            src = (y, x - 1)
        elif r < 6 and y > 0 and not flags[y - 1, x] & U_INTRA:
            src = (y - 1, x)
        if src is not None and flags[src] & (U_PRED_L0 | U_PRED_L1):   # merge: the neighbour's motion, now and then refined
            f = int(flags[src]) & (U_PRED_L0 | U_PRED_L1)
            d = rng.integers(-4, 5, 2) if rng.integers(0, 3) == 0 else 0
            for l in (0, 1):
                rect(mv[l], x, y, bw, bh, np.clip(mv[l][src] + d, INT16_MIN, INT16_MAX))
                rect(ref[l], x, y, bw, bh, ref[l][src])
        else:
            f = (U_PRED_L0, U_PRED_L1, U_PRED_L0 | U_PRED_L1)[rng.integers(0, 3)]
            for l in (0, 1):
                if f & (U_PRED_L0, U_PRED_L1)[l]:
                    rect(mv[l], x, y, bw, bh, rng.integers(-64, 65, 2))
                    rect(ref[l], x, y, bw, bh, pocs[rng.integers(0, len(pocs))])
        flags[y:y + bh, x:x + bw] |= f

    def transform_tree(x, y, s, depth, p_cbf):
        if s > 1 and (s > 8 or rng.integers(0, 10) < (5 if depth == 0 else 3)):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    transform_tree(x + dx, y + dy, s // 2, depth + 1, p_cbf)
            return
        flags[y:y + s, x] |= U_TU_LEFT
        flags[y, x:x + s] |= U_TU_TOP
        if rng.integers(0, 100) < p_cbf:
            flags[y:y + s, x:x + s] |= U_CBF

    def coding_unit(x, y, s, extra):
        intra = rng.integers(0, 4) == 0
        special = rng.integers(0, 20) == 0                 # PCM with the loop filter off / transquant bypass
        rect(flags, x, y, s, s, extra | (U_INTRA if intra else 0) | (U_KEEP if special else 0))
        q = s // 4
        if intra:
            part = rng.integers(0, 2) if s == 2 else 0     # NxN at the smallest size only
            parts = [(0, 0, s, s)] if part == 0 else [(0, 0, 1, 1), (1, 0, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1)]
        else:
            part = rng.integers(0, 8 if s >= 4 else 4)
            hs = s // 2
            parts = {0: [(0, 0, s, s)], 1: [(0, 0, s, hs), (0, hs, s, hs)], 2: [(0, 0, hs, s), (hs, 0, hs, s)],
                     3: [(0, 0, hs, hs), (hs, 0, hs, hs), (0, hs, hs, hs), (hs, hs, hs, hs)]}.get(part)
            if parts is None:                              # asymmetric: the inner edge at a quarter of the block
                parts = {4: [(0, 0, s, q), (0, q, s, s - q)], 5: [(0, 0, s, s - q), (0, s - q, s, q)],
                         6: [(0, 0, q, s), (q, 0, s - q, s)], 7: [(0, 0, s - q, s), (s - q, 0, q, s)]}[part]
        for (dx, dy, bw, bh) in parts:
            pred_block(x + dx, y + dy, bw, bh, intra)
        skip = not intra and part == 0 and rng.integers(0, 3) == 0
        if skip:
            flags[y:y + s, x] |= U_TU_LEFT
            flags[y, x:x + s] |= U_TU_TOP
        else:
            transform_tree(x, y, s, 0, 60 if intra else 35)

    def quadtree(x, y, s, extra):
        if x >= uw or y >= uh:
            return
        must = x + s > uw or y + s > uh
        if s > 2 and (must or rng.integers(0, 10) < {16: 9, 8: 6, 4: 4}[s]):
            for dy in (0, s // 2):
                for dx in (0, s // 2):
                    quadtree(x + dx, y + dy, s // 2, extra)
            return
        coding_unit(x, y, s, extra)

    for cy in range(chh):
        for cx in range(cw):
            sl = int(slice_of[cy, cx])
            quadtree(cx * cs, cy * cs, cs, U_DBK_OFF if slice_off[sl] else 0)
    # borders in-loop filtering must not cross (the flag of the slice holding the Q side decides; tiles: one PPS flag)
    for cy in range(chh):
        for cx in range(cw):
            sl = int(slice_of[cy, cx])
            ys, xs = slice(cy * cs, min((cy + 1) * cs, uh)), slice(cx * cs, min((cx + 1) * cs, uw))
            if cx > 0 and ((slice_nox[sl] and slice_of[cy, cx - 1] != sl) or (tiles_nox and cx in tile_cols)):
                flags[ys, cx * cs] |= U_NOX_LEFT
            if cy > 0 and ((slice_nox[sl] and slice_of[cy - 1, cx] != sl) or (tiles_nox and cy in tile_rows)):
                flags[cy * cs, xs] |= U_NOX_TOP
    return tuple(np.ascontiguousarray(a).astype(dt) for a, dt in zip((flags, mv[0], mv[1], ref[0], ref[1]), UNIT_DTYPES))


# ---- transformations under which the rule is invariant (metamorphic checks) -------------------------------------------

def transpose_units(units):
    """the picture mirrored at its diagonal: unit arrays transposed, x / y of every vector and LEFT / TOP of every flag swapped"""
    f = np.asarray(units[0]).astype(np.int64)
    g = f & ~(U_TU_LEFT | U_TU_TOP | U_PU_LEFT | U_PU_TOP | U_NOX_LEFT | U_NOX_TOP)
    for a, b in ((U_TU_LEFT, U_TU_TOP), (U_PU_LEFT, U_PU_TOP), (U_NOX_LEFT, U_NOX_TOP)):
        g |= np.where(f & a, b, 0) | np.where(f & b, a, 0)
    out = [g.T.astype(np.uint16)] + [np.swapaxes(np.asarray(m), 0, 1)[..., ::-1] for m in units[1:3]] + [np.asarray(r).T for r in units[3:5]]
    return tuple(np.ascontiguousarray(a) for a in out)


def swap_lists(units):
    """list 0 and list 1 of every unit exchanged"""
    f = np.asarray(units[0]).astype(np.int64)
    g = (f & ~(U_PRED_L0 | U_PRED_L1)) | np.where(f & U_PRED_L0, U_PRED_L1, 0) | np.where(f & U_PRED_L1, U_PRED_L0, 0)
    return (g.astype(np.uint16), units[2], units[1], units[4], units[3])
