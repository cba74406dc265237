"""Test vectors for the spec-exact mode at its decision edges, and an independent numpy restatement of its luma filter.

TEST INFRASTRUCTURE ONLY.  Two things live here:

* luma_reference(): H.265 clauses 8.7.2.5.3 (decisions), 8.7.2.5.6 (dSam) and 8.7.2.5.7 (luma filter) restated in numpy
  int64 from the clause text, in picture order (every vertical edge, then every horizontal edge on the result).  It shares
  nothing with oracle/h265_oracle.c but the tables, and besides the filtered plane it reports what happened: a label per
  4-line segment, which clips fired and which thresholds were met exactly at value - 1 and at value.
* constructive generators: planes whose segments are solved to land on a chosen decision, exactly on either side of a
  threshold, or at the extremes of the sample range (luma_edge_plane, chroma_edge_plane), and full-range SAO content with
  parameters that reach every band position, edge class and offset magnitude (sao_full_range).

Everything is generated from a numpy Generator, so a test needs no stored vectors.
"""
from collections import Counter

import numpy as np

import rext_oracle as rx

BS_MASK, KEEP_P, KEEP_Q = 3, 4, 8

# Table 8-12
BETA_TABLE = np.array([0] * 16 + [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42,
                       44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64], np.int64)
TC_TABLE = rx.TC_TABLE
assert BETA_TABLE.size == 52

LABELS = ("off_bs0", "off_d", "strong", "normal_p0q0", "normal_p0q1", "normal_p1q0", "normal_p1q1", "normal_skipped")
BOUNDARY = -1  # label of the picture-boundary entries of the bS arrays (never filtered)
CLIP_KINDS = tuple("clip1_%s_%s" % (s, e) for s in ("p0", "q0", "p1", "q1") for e in ("lo", "hi")) + \
    tuple("clamp_%s_%s" % (s, e) for s in ("p0", "p1", "p2", "q0", "q1", "q2") for e in ("lo", "hi"))
THRESHOLDS = ("d", "dpq0", "dpq3", "e0", "e3", "f0", "f3", "dEp", "dEq", "delta")


def beta_tc(qpl, bs, bit_depth, tc_offset_div2=0, beta_offset_div2=0):
    """8.7.2.5.3: beta and tC of a luma edge with QpL qpl and boundary strength bs (arrays allowed)"""
    qpl, bs = np.asarray(qpl, np.int64), np.asarray(bs, np.int64)
    beta = BETA_TABLE[np.clip(qpl + 2 * beta_offset_div2, 0, 51)] << (bit_depth - 8)
    tc = TC_TABLE[np.clip(qpl + 2 * (bs - 1) + 2 * tc_offset_div2, 0, 53)] << (bit_depth - 8)
    return beta, tc


def max_ramp_numerator(bit_depth):
    """the largest 9 * (q0 - p0) - 3 * (q1 - p1) + 8 on legal content with d = 0: p = 0, a, 2a, 3a | q = M, M - a, .. with
    a = M // 3 (32768 at 12 bit)"""
    m = (1 << bit_depth) - 1
    return 6 * m + 6 * (m // 3) + 8


# ---- the reference ----------------------------------------------------------------------------------------------------

def _edge_pass(s, bs, qp_of, bit_depth, tc_offset_div2, beta_offset_div2, st):
    """every vertical edge x = 8k (0 < x < W) of s (H x W, int64, modified in place); bs = (H/4, W/8+1) entries;
    qp_of(x, y) = QpY of the coding unit holding sample (x, y).  Returns the (H/4, W/8+1) labels."""
    H, W = s.shape
    n4 = H // 4
    labels = np.full((n4, W // 8 + 1), BOUNDARY, np.int64)
    xs = np.arange(8, W, 8)
    if not xs.size or not n4:
        return labels
    max_v = (1 << bit_depth) - 1
    ne = xs.size
    ent = np.asarray(bs, np.int64).reshape(n4, W // 8 + 1)[:, xs // 8]
    b = ent & BS_MASK
    y0 = (np.arange(n4) * 4)[:, None]
    qpl = (qp_of(xs[None, :], y0) + qp_of(xs[None, :] - 1, y0) + 1) >> 1
    beta, tc = beta_tc(qpl, b, bit_depth, tc_offset_div2, beta_offset_div2)
    # taps: P[k][line] = p_k of that line, shape (H, nE)
    P = [s[:, xs - 1 - k].copy() for k in range(4)]
    Q = [s[:, xs + k].copy() for k in range(4)]

    def line(a, i):  # line i (0..3) of every segment: (n4, nE)
        return a[i::4]
    dp = {i: np.abs(line(P[2], i) - 2 * line(P[1], i) + line(P[0], i)) for i in (0, 3)}
    dq = {i: np.abs(line(Q[2], i) - 2 * line(Q[1], i) + line(Q[0], i)) for i in (0, 3)}
    dpq = {i: dp[i] + dq[i] for i in (0, 3)}
    d = dpq[0] + dpq[3]
    on = b != 0
    de_on = on & (d < beta)                                   # dE != 0
    t_dpq, t_e, t_f = beta >> 2, beta >> 3, (5 * tc + 1) >> 1
    e = {i: np.abs(line(P[3], i) - line(P[0], i)) + np.abs(line(Q[0], i) - line(Q[3], i)) for i in (0, 3)}
    f = {i: np.abs(line(P[0], i) - line(Q[0], i)) for i in (0, 3)}
    c1 = {i: 2 * dpq[i] < t_dpq for i in (0, 3)}
    c2 = {i: e[i] < t_e for i in (0, 3)}
    c3 = {i: f[i] < t_f for i in (0, 3)}
    dsam = {i: c1[i] & c2[i] & c3[i] for i in (0, 3)}
    strong = de_on & dsam[0] & dsam[3]                        # dE = 2
    normal = de_on & ~strong                                  # dE = 1
    side = (beta + (beta >> 1)) >> 3
    dEp = (dp[0] + dp[3]) < side
    dEq = (dq[0] + dq[3]) < side

    def ev(name, x, t, where, step=1):
        """threshold met exactly: the largest passing value (x < t, x + step >= t) and the smallest failing one"""
        st["events"][(name, "below")] += int(np.count_nonzero(where & (x < t) & (x + step >= t)))
        st["events"][(name, "at")] += int(np.count_nonzero(where & (x >= t) & (x - step < t)))
    ev("d", d, beta, on)
    for i, j in ((0, 3), (3, 0)):   # decisive: the other two conditions of the line and the other line's dSam hold
        ev("dpq%d" % i, 2 * dpq[i], t_dpq, de_on & c2[i] & c3[i] & dsam[j], 2)
        ev("e%d" % i, e[i], t_e, de_on & c1[i] & c3[i] & dsam[j])
        ev("f%d" % i, f[i], t_f, de_on & c1[i] & c2[i] & dsam[j])
    ev("dEp", dp[0] + dp[3], side, normal)
    ev("dEq", dq[0] + dq[3], side, normal)
    ext = st["extras"]
    filt = on & (tc >= 0)
    ext["tc_max"] += int(np.count_nonzero(de_on & (tc == 24 << (bit_depth - 8))))
    ext["beta_max"] += int(np.count_nonzero(on & (beta == 64 << (bit_depth - 8))))
    ext["beta_sh3_0"] += int(np.count_nonzero(filt & (t_e == 0) & (beta > 0)))
    ext["beta_sh3_1"] += int(np.count_nonzero(filt & (t_e == 1)))
    ext["beta_sh2_0"] += int(np.count_nonzero(filt & (t_dpq == 0) & (beta > 0)))
    ext["beta_sh2_1"] += int(np.count_nonzero(filt & (t_dpq == 1)))
    ext["tc0_beta_pos"] += int(np.count_nonzero(de_on & (tc == 0)))

    # per line: segment values repeated over its four lines
    def rep(a):
        return np.repeat(a, 4, axis=0)
    tcL, strongL, normalL, dEpL, dEqL = rep(tc), rep(strong), rep(normal), rep(dEp), rep(dEq)
    keep_p, keep_q = rep((ent & KEEP_P) != 0), rep((ent & KEEP_Q) != 0)
    p0, p1, p2, p3 = P
    q0, q1, q2, q3 = Q
    # 8.7.2.5.7, dE == 2
    raw = {"p0": (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3, "p1": (p2 + p1 + p0 + q0 + 2) >> 2,
           "p2": (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3, "q0": (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3,
           "q1": (p0 + q0 + q1 + q2 + 2) >> 2, "q2": (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3}
    orig = {"p0": p0, "p1": p1, "p2": p2, "q0": q0, "q1": q1, "q2": q2}
    sums_max = (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) == 8 * max_v + 4
    ext["strong_sum_max"] += int(np.count_nonzero(strongL & sums_max))
    new = dict(orig)
    for k in raw:
        keep = keep_p if k[0] == "p" else keep_q
        lo, hi = orig[k] - 2 * tcL, orig[k] + 2 * tcL
        st["clips"]["clamp_%s_lo" % k] += int(np.count_nonzero(strongL & ~keep & (raw[k] < lo)))
        st["clips"]["clamp_%s_hi" % k] += int(np.count_nonzero(strongL & ~keep & (raw[k] > hi)))
        new[k] = np.where(strongL, np.clip(raw[k], lo, hi), new[k])
    # dE == 1
    num = 9 * (q0 - p0) - 3 * (q1 - p1) + 8
    delta = num >> 4
    ext["max_ramp"] += int(np.count_nonzero(normalL & (np.abs(num - 8) == max_ramp_numerator(bit_depth) - 8)))
    ev("delta", np.abs(delta), 10 * tcL, normalL)
    apply = normalL & (np.abs(delta) < 10 * tcL)
    dc = np.clip(delta, -tcL, tcL)
    cand = {"p0": p0 + dc, "q0": q0 - dc,
            "p1": p1 + np.clip((((p2 + p0 + 1) >> 1) - p1 + dc) >> 1, -(tcL >> 1), tcL >> 1),
            "q1": q1 + np.clip((((q2 + q0 + 1) >> 1) - q1 - dc) >> 1, -(tcL >> 1), tcL >> 1)}
    gate = {"p0": apply & ~keep_p, "q0": apply & ~keep_q, "p1": apply & dEpL & ~keep_p, "q1": apply & dEqL & ~keep_q}
    for k, v in cand.items():
        st["clips"]["clip1_%s_lo" % k] += int(np.count_nonzero(gate[k] & (v < 0)))
        st["clips"]["clip1_%s_hi" % k] += int(np.count_nonzero(gate[k] & (v > max_v)))
        use = apply & ((dEpL if k == "p1" else dEqL) if k[1] == "1" else True)
        new[k] = np.where(use, np.clip(v, 0, max_v), new[k])
    # nDp / nDq = 0 leave the side as it was
    for k in new:
        new[k] = np.where(keep_p if k[0] == "p" else keep_q, orig[k], new[k])
    for k in range(3):
        s[:, xs - 1 - k] = new["p%d" % k]
        s[:, xs + k] = new["q%d" % k]
    # labels
    skipped = normal & ~np.any((np.abs(delta) < 10 * tcL).reshape(n4, 4, ne), axis=1)
    lab = np.where(~on, 0, np.where(~de_on, 1, np.where(strong, 2, np.where(skipped, 7, 3 + 2 * dEp + dEq))))
    labels[:, xs // 8] = lab
    for i, name in enumerate(LABELS):
        st["labels"][name] += int(np.count_nonzero(lab == i))
    return labels


def new_stats():
    return {"labels": Counter(), "clips": Counter(), "events": Counter(), "extras": Counter()}


def merge_stats(a, b):
    for k in a:
        a[k].update(b[k])
    return a


def luma_reference(plane, qp, vb, hb, *, bit_depth=8, qp_map=None, unit_log2=3, tc_offset_div2=0, beta_offset_div2=0, stats=None):
    """8.7.2 for a luma plane (H x W, multiples of 8): vertical edges of the picture, then horizontal edges on the result.
    vb: (W/8+1) x (H/4) entries, hb: (H/8+1) x (W/4) (bits 1:0 bS, bit 2 / 3 keep P / Q); qp_map[y >> unit_log2, x >> unit_log2]
    = QpY, or the scalar qp.  Returns (filtered plane, {"vert": labels, "hor": labels, "stats": ...}); labels index LABELS
    (BOUNDARY on the picture edges), stats counts labels, clips (CLIP_KINDS), threshold events ((name, "below" | "at"))."""
    src = np.asarray(plane)
    s = src.astype(np.int64)
    H, W = s.shape
    st = new_stats() if stats is None else stats
    if qp_map is None:
        def qv(x, y):
            return np.full(np.broadcast(x, y).shape, int(qp), np.int64)
        qh = qv
    else:
        m = np.asarray(qp_map, np.int64)

        def qv(x, y):
            return m[y >> unit_log2, x >> unit_log2]

        def qh(x, y):  # transposed coordinates
            return m[x >> unit_log2, y >> unit_log2]
    vert = _edge_pass(s, np.asarray(vb).reshape(H // 4, W // 8 + 1), qv, bit_depth, tc_offset_div2, beta_offset_div2, st)
    t = np.ascontiguousarray(s.T)
    hor = _edge_pass(t, np.asarray(hb).reshape(H // 8 + 1, W // 4).T, qh, bit_depth, tc_offset_div2, beta_offset_div2, st)
    return t.T.astype(src.dtype), {"vert": vert, "hor": hor.T, "stats": st}


# ---- luma vectors -----------------------------------------------------------------------------------------------------

def _line(a, g, sp=0, cp=0, ep=0, sq=0, cq=0, eq=0):
    """p3 p2 p1 p0 | q0 q1 q2 q3 with p0 = a, q0 = a + g; slope s, curvature c (= dp / dq), extra step e of p3 / q3"""
    p1 = a + sp
    p2 = a + 2 * sp + cp
    p3 = p2 + sp + ep
    q0 = a + g
    q1 = q0 + sq
    q2 = q0 + 2 * sq + cq
    q3 = q2 + sq + eq
    return [p3, p2, p1, a, q0, q1, q2, q3]


def _split(rng, total, n):
    """n non-negative integers summing to total"""
    if total <= 0:
        return [0] * n
    cuts = np.sort(rng.integers(0, total + 1, n - 1))
    return list(np.diff(np.concatenate([[0], cuts, [total]])))


def _sgn(rng):
    return 1 if rng.integers(0, 2) else -1


class _Builder:
    """solves one segment's 4 x 8 samples for a case; counters make consecutive uses alternate the threshold side and line"""

    CASES = ("d", "dpq", "e", "f", "dE", "delta", "clip", "clamp", "maxramp", "summax", "texture")

    def __init__(self, rng, bit_depth):
        self.rng, self.bd = rng, bit_depth
        self.max_v = (1 << bit_depth) - 1
        self.n = Counter()

    def _flip(self, seg, mirror=None, swap=None):
        r = self.rng
        if mirror if mirror is not None else r.integers(0, 2):
            seg = self.max_v - seg
        if swap if swap is not None else r.integers(0, 2):
            seg = seg[:, ::-1]
        return seg

    def _place(self, lines, small=0):
        """relative lines -> absolute 4 x 8 at a random level (None if they do not fit); lines 1, 2 copy lines 0, 3"""
        seg = np.array([lines[0], lines[0], lines[1], lines[1]], np.int64)
        lo, hi = seg.min(), seg.max()
        if hi - lo > self.max_v:
            return None
        base = int(self.rng.integers(0, self.max_v - (hi - lo) + 1)) - lo
        return self._flip(seg + base)

    def _side(self, name):
        self.n[name] += 1
        return self.n[name] % 2  # 0: value - 1, 1: value

    def _small_g(self, tf):
        return int(self.rng.integers(-(tf - 1), tf)) if tf > 1 else 0

    def build(self, case, beta, tc):
        r, sh = self.rng, self.bd - 8
        tf = (5 * tc + 1) >> 1
        flat = lambda: _line(0, self._small_g(tf))
        if case == "d":
            if beta < 1:
                return None
            D = beta - 1 + self._side("d")
            parts = _split(r, D, 4)
            ls = []
            for k in (0, 2):
                cp, cq = parts[k] * _sgn(r), parts[k + 1] * _sgn(r)
                ls.append(_line(0, self._small_g(tf), cp=cp, ep=-cp, cq=cq, eq=-cq))
            return self._place(ls)
        if case == "dpq":
            t = ((beta >> 2) + 1) >> 1  # 2 * dpq < beta >> 2  <=>  dpq < t
            if t < 1:
                return None
            x = t - 1 + self._side("dpq")
            a, b = _split(r, x, 2)
            cp, cq = a * _sgn(r), b * _sgn(r)
            ln = _line(0, self._small_g(tf), cp=cp, ep=-cp, cq=cq, eq=-cq)
            self.n["dpq_line"] += 1
            return self._place([ln, flat()] if (self.n["dpq_line"] // 2) % 2 else [flat(), ln])
        if case == "e":
            te = beta >> 3
            if te < 1:
                return None
            x = te - 1 + self._side("e")
            a, b = _split(r, x, 2)
            ln = _line(0, self._small_g(tf), ep=a * _sgn(r), eq=b * _sgn(r))
            self.n["e_line"] += 1
            return self._place([ln, flat()] if (self.n["e_line"] // 2) % 2 else [flat(), ln])
        if case == "f":
            if tf < 1:
                return None
            x = tf - 1 + self._side("f")
            ln = _line(0, x * _sgn(r))
            self.n["f_line"] += 1
            return self._place([ln, flat()] if (self.n["f_line"] // 2) % 2 else [flat(), ln])
        if case == "dE":
            side = (beta + (beta >> 1)) >> 3
            if side < 1:
                return None
            xp = side - 1 + self._side("dEp")
            xq = [side - 1, side, 0, int(r.integers(0, side + 1))][self.n["dE"] % 4]
            self.n["dE"] += 1
            ap, bp = _split(r, xp, 2)
            aq, bq = _split(r, xq, 2)
            ls = []
            for cp, cq in ((ap, aq), (bp, bq)):
                cp, cq = cp * _sgn(r), cq * _sgn(r)
                g = max(tf, 1) + int(r.integers(0, max(tf, 1) + 1))
                ls.append(_line(0, g * _sgn(r), cp=cp, ep=-cp, cq=cq, eq=-cq))
            return self._place(ls)
        if case == "delta":
            K = 10 * tc - 1 + self._side("delta")
            if K < 1:
                return None
            mirror, swap = bool(r.integers(0, 2)), bool(r.integers(0, 2))
            # numerator N = 9 (q0 - p0) - 3 (q1 - p1) + 8 of the built line; mirror or swap alone turn it into 16 - N
            lo, hi = (16 * K + 1, 16 * K + 16) if mirror != swap else (16 * K, 16 * K + 15)
            for _ in range(40):
                a = int(r.integers(0, self.max_v // 3 + 1))
                b = int(r.integers(0, self.max_v // 3 + 1))
                s3 = 3 * (a + b) + 8
                g = -((-(lo - s3)) // 6)
                if 6 * g + s3 > hi:
                    continue
                amin, amax = max(0, 3 * b - g), min(self.max_v - 3 * a, self.max_v - g)
                if amin > amax:
                    continue
                A = int(r.integers(amin, amax + 1))
                ln = np.array(_line(A, g, sp=a, sq=-b), np.int64)
                return self._flip(np.array([ln] * 4), mirror, swap)
            return None
        if case == "clip":
            if tc < 1 or beta < 1:
                return None
            c = int(r.integers(0, tc))
            q0 = int(r.integers(0, c + 1))
            smin = max(2 * tc, (beta >> 3) // 3 + 1, 1)
            smax = min(self.max_v // 3 - q0, 50 * tc)
            if smin > smax:
                return None
            s = int(r.integers(smin, smax + 1))
            ln = np.array([c, c, c, c, q0, q0 + s, q0 + 2 * s, q0 + 3 * s], np.int64)
            return self._flip(np.array([ln] * 4))
        if case == "clamp":
            return self._clamp(beta, tc)
        if case == "maxramp":
            a = self.max_v // 3
            ln = np.array(_line(0, self.max_v, sp=a, sq=-a), np.int64)
            return self._flip(np.array([ln] * 4))
        if case == "summax":
            return self._flip(np.full((4, 8), self.max_v, np.int64), mirror=False)
        # texture: a step between two noisy plateaus
        g = int(r.integers(-4 * max(tc, 1), 4 * max(tc, 1) + 1))
        seg = np.array([[0] * 4 + [g] * 4] * 4, np.int64) + (r.integers(-6, 7, (4, 8)) << sh)
        return self._place([seg[0], seg[3]])

    def _clamp(self, beta, tc):
        """strong-filter content (every dSam condition just met) whose unclamped outputs leave +-2 tC: random search"""
        r = self.rng
        td, te, tf = ((beta >> 2) - 1) // 2, (beta >> 3) - 1, ((5 * tc + 1) >> 1) - 1
        if td < 0 or te < 0 or tf < 0 or tc < 1:
            return None
        n = 256
        R = max(te, tf, 1)
        sp, sq = r.integers(-R, R + 1, n), r.integers(-R, R + 1, n)
        cp = r.integers(0, td + 1, n)
        cq = np.array([int(r.integers(0, td - c + 1)) for c in cp])
        cp, cq = cp * np.where(r.integers(0, 2, n) > 0, 1, -1), cq * np.where(r.integers(0, 2, n) > 0, 1, -1)
        ea = r.integers(0, te + 1, n)
        eb = np.array([int(r.integers(0, te - x + 1)) for x in ea])
        ep = ea * np.where(r.integers(0, 2, n) > 0, 1, -1) - 3 * sp - cp   # |p3 - p0| = ea
        eq = eb * np.where(r.integers(0, 2, n) > 0, 1, -1) - 3 * sq - cq
        g = r.integers(-tf, tf + 1, n)
        L = np.array(_line(np.zeros(n, np.int64), g, sp, cp, ep, sq, cq, eq))  # (8, n)
        p3, p2, p1, p0, q0, q1, q2, q3 = L
        outs = [((p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3) - p0, ((p2 + p1 + p0 + q0 + 2) >> 2) - p1,
                ((2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3) - p2, ((p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3) - q0,
                ((p0 + q0 + q1 + q2 + 2) >> 2) - q1, ((p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3) - q2]
        k = self.n["clamp"] % 12
        self.n["clamp"] += 1
        # the filter is symmetric under p <-> q: a Q-side target is the P-side one, reversed
        o = np.asarray(outs[(k // 2) % 3])
        hit = np.nonzero(o < -2 * tc if k % 2 == 0 else o > 2 * tc)[0]
        if not hit.size:
            hit = np.nonzero(np.max(np.abs(np.array(outs)), axis=0) > 2 * tc)[0]
            if not hit.size:
                return None
        ln = L[:, hit[0]]
        seg = np.array([ln] * 4, np.int64)
        if k >= 6:
            seg = seg[:, ::-1]
        lo, hi = seg.min(), seg.max()
        if hi - lo > self.max_v:
            return None
        return seg + int(r.integers(0, self.max_v - (hi - lo) + 1)) - lo   # no mirror: keeps the wanted direction


WAVE_MODES = ("bs2", "bs1", "mixed", "keep")


def _wave_bs(rng, mode):
    if rng.integers(0, 8) == 0:
        return 0
    if mode == "bs2":
        return 2
    if mode == "bs1":
        return 1
    b = int(rng.integers(1, 3))
    if mode == "keep":
        b |= (KEEP_P, KEEP_Q, KEEP_P | KEEP_Q, 0)[int(rng.integers(0, 4))]
    return b


def luma_edge_plane(bit_depth, qp, tc_offset_div2, beta_offset_div2, rng, *, w=1056, h=32, direction="v", qp_map=None, unit_log2=3):
    """A w x h luma plane whose edge segments of one direction are each solved for a case of _Builder.CASES, with the bS arrays
    (the other direction all 0).  direction "v": vertical edges; the 8 samples p3..q3 of a segment are disjoint from every
    other segment's.  direction "h": the transposed twin (horizontal edges, vertical bS 0).  bS runs: along a block row, the 64
    blocks of a wave of the packed kernels are uniform bS 2, uniform bS 1, mixed 1 / 2, or carry keep flags (WAVE_MODES, a
    few bS 0 everywhere).  tC and beta of a segment follow from qp, or from qp_map[y >> unit_log2, x >> unit_log2]."""
    if direction == "h":
        m = None if qp_map is None else np.ascontiguousarray(np.asarray(qp_map).T)
        p, vb, hb = luma_edge_plane(bit_depth, qp, tc_offset_div2, beta_offset_div2, rng, w=h, h=w, qp_map=m, unit_log2=unit_log2)
        vbT = vb.reshape(w // 4, h // 8 + 1)
        return np.ascontiguousarray(p.T), np.zeros((w // 8 + 1) * (h // 4), np.uint8), np.ascontiguousarray(vbT.T).ravel()
    assert w % 8 == 0 and h % 8 == 0
    max_v = (1 << bit_depth) - 1
    plane = rng.integers(max_v // 4, 3 * max_v // 4 + 1, (h, w)).astype(np.int64)
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    bld = _Builder(rng, bit_depth)
    m = None if qp_map is None else np.asarray(qp_map, np.int64)
    k = int(rng.integers(0, len(_Builder.CASES)))
    for y4 in range(h // 4):
        for bx in range(1, w // 8):
            ent = _wave_bs(rng, WAVE_MODES[(y4 // 2 + bx // 64) % 4])
            vb[y4, bx] = ent
            x = 8 * bx
            qpl = int(qp) if m is None else (int(m[(4 * y4) >> unit_log2, x >> unit_log2]) +
                                             int(m[(4 * y4) >> unit_log2, (x - 1) >> unit_log2]) + 1) >> 1
            beta, tc = beta_tc(qpl, max(ent & BS_MASK, 1), bit_depth, tc_offset_div2, beta_offset_div2)
            seg = None
            for _ in range(len(_Builder.CASES)):
                seg = bld.build(_Builder.CASES[k % len(_Builder.CASES)], int(beta), int(tc))
                k += 1
                if seg is not None:
                    break
            if seg is None:
                seg = bld.build("texture", int(beta), int(tc))
            assert seg.min() >= 0 and seg.max() <= max_v
            plane[4 * y4:4 * y4 + 4, x - 4:x + 4] = seg
    return plane.astype(np.uint8 if bit_depth == 8 else np.uint16), vb.ravel(), np.zeros((h // 8 + 1) * (w // 4), np.uint8)


def all_qp_map(w, h, unit_log2, rng, lo=0, hi=51):
    """a QP map whose units take every QP in lo..hi, shuffled"""
    n = (-(-h >> unit_log2)) * (-(-w >> unit_log2))
    v = np.resize(np.arange(lo, hi + 1), n)
    rng.shuffle(v)
    return v.reshape(-(-h >> unit_log2), -(-w >> unit_log2)).astype(np.uint8)


# ---- chroma vectors ---------------------------------------------------------------------------------------------------

def chroma_edge_plane(bit_depth, rng, *, w=528, h=32, chroma_format=1, qp=37, qp_map=None, unit_log2=3, c_qp_offset=0,
                      tc_offset_div2=0, direction="v"):
    """A chroma plane (w x h in its own geometry) whose vertical (or, "h", horizontal) edge segments put the chroma filter
    (8.7.2.5.8) at its ends: the delta clip at +-tC, Clip1 at 0 and max_v on p0 and q0, small deltas, bS 1 / 0 and keep
    flags.  tC per segment from qp or qp_map (QpY per luma unit) as rext_oracle derives it.  Returns plane, vb, hb."""
    sx, sy = rx.SUB[chroma_format]
    if direction == "h":
        # transpose the problem: the QP of chroma sample (x, y) is read at luma (x sx, y sy)
        m = None if qp_map is None else np.ascontiguousarray(np.asarray(qp_map).T)
        p, vb, hb = _chroma_plane(bit_depth, rng, h, w, sy, sx, qp, m, unit_log2, c_qp_offset, tc_offset_div2, chroma_format)
        vbT = vb.reshape(w // 4, h // 8 + 1)
        return np.ascontiguousarray(p.T), np.zeros((w // 8 + 1) * (h // 4), np.uint8), np.ascontiguousarray(vbT.T).ravel()
    return _chroma_plane(bit_depth, rng, w, h, sx, sy, qp, qp_map, unit_log2, c_qp_offset, tc_offset_div2, chroma_format)


def _chroma_plane(bd, rng, w, h, sx, sy, qp, qp_map, unit_log2, c_qp_offset, tc_offset_div2, cf):
    max_v = (1 << bd) - 1
    plane = rng.integers(max_v // 4, 3 * max_v // 4 + 1, (h, w)).astype(np.int64)
    vb = np.zeros((h // 4, w // 8 + 1), np.uint8)
    m = None if qp_map is None else np.asarray(qp_map, np.int64)
    lw, lh = w * sx, h * sy
    n = 0
    for y4 in range(h // 4):
        for bx in range(1, w // 8):
            x = 8 * bx
            r = int(rng.integers(0, 16))
            ent = 0 if r == 0 else 1 if r == 1 else 2
            if rng.integers(0, 10) == 0:
                ent |= (KEEP_P, KEEP_Q)[int(rng.integers(0, 2))]
            vb[y4, bx] = ent
            if m is None:
                qpl = min(int(qp), 51)
            else:
                def at(cx, cy):
                    return int(m[min(cy * sy, lh - 1) >> unit_log2, min(cx * sx, lw - 1) >> unit_log2])
                qpl = min((at(x, 4 * y4) + at(x - 1, 4 * y4) + 1) >> 1, 51)
            tc = int(rx.chroma_tc(qpl, cf, c_qp_offset=c_qp_offset, tc_offset_div2=tc_offset_div2, bit_depth=bd))
            case = n % 4
            n += 1
            if case == 0:    # |delta| beyond tC: delta = ((q0 - p0) * 4 + p1 - q1 + 4) >> 3 with a plain step
                g = max(2 * tc + 2, 4) + int(rng.integers(0, 4 * max(tc, 1) + 1))
                g = min(g, max_v)
                base = int(rng.integers(0, max_v - g + 1))
                ln = [base] * 4 + [base + g] * 4
            elif case == 1:  # Clip1: p0 at the bottom, the Q side rising steeply
                c = int(rng.integers(0, max(tc, 1)))
                s = int(rng.integers(8 * max(tc, 1), max(8 * max(tc, 1), max_v // 3) + 1))
                s = min(s, max_v // 3)
                ln = [c] * 4 + [0, s, 2 * s, 3 * s]
            elif case == 2:  # small steps: delta inside +-tC
                g = int(rng.integers(-max(tc, 1), max(tc, 1) + 1))
                base = int(rng.integers(abs(g), max_v - abs(g) + 1))
                ln = [base] * 4 + [base + g] * 4
            else:            # a step at full range
                ln = [0] * 4 + [max_v] * 4
            seg = np.array([ln] * 4, np.int64) + rng.integers(0, 2, (4, 8))
            seg = np.clip(seg, 0, max_v)
            if rng.integers(0, 2):
                seg = max_v - seg
            if rng.integers(0, 2):
                seg = seg[:, ::-1]
            plane[4 * y4:4 * y4 + 4, x - 4:x + 4] = seg
    return plane.astype(np.uint8 if bd == 8 else np.uint16), vb.ravel(), np.zeros((h // 8 + 1) * (w // 4), np.uint8)


def chroma_events(plane, vb, chroma_format, *, bit_depth=8, qp=37, qp_map=None, unit_log2=3, c_qp_offset=0, tc_offset_div2=0):
    """what the vertical edges of a chroma plane (8.7.2.5.8, bS 2) do: Counter of tc_clip_lo / _hi (|delta| beyond tC),
    clip1_p0_lo / _hi, clip1_q0_lo / _hi, and the qPi values (("qpi", v)) of the filtered segments"""
    sx, sy = rx.SUB[chroma_format]
    s = np.asarray(plane, np.int64)
    ch, cw = s.shape
    max_v = (1 << bit_depth) - 1
    ev = Counter()
    xs = np.arange(8, cw, 8)
    if not xs.size:
        return ev
    ent = np.asarray(vb, np.int64).reshape(ch // 4, cw // 8 + 1)[:, xs // 8]
    y0 = (np.arange(ch // 4) * 4)[:, None]
    qpp = rx._qp_at(qp, qp_map, unit_log2, (xs[None, :] - 1) * sx, y0 * sy, cw * sx, ch * sy)
    qpq = rx._qp_at(qp, qp_map, unit_log2, xs[None, :] * sx, y0 * sy, cw * sx, ch * sy)
    qpl = np.minimum((qpp + qpq + 1) >> 1, 51)
    tc = np.repeat(rx.chroma_tc(qpl, chroma_format, c_qp_offset=c_qp_offset, tc_offset_div2=tc_offset_div2, bit_depth=bit_depth), 4, 0)
    on = np.repeat((ent & BS_MASK) == 2, 4, 0)
    kp, kq = np.repeat((ent & KEEP_P) != 0, 4, 0), np.repeat((ent & KEEP_Q) != 0, 4, 0)
    p1, p0, q0, q1 = s[:, xs - 2], s[:, xs - 1], s[:, xs], s[:, xs + 1]
    raw = ((q0 - p0) * 4 + p1 - q1 + 4) >> 3
    d = np.clip(raw, -tc, tc)
    ev["tc_clip_lo"] += int(np.count_nonzero(on & (raw < -tc)))
    ev["tc_clip_hi"] += int(np.count_nonzero(on & (raw > tc)))
    ev["clip1_p0_lo"] += int(np.count_nonzero(on & ~kp & (p0 + d < 0)))
    ev["clip1_p0_hi"] += int(np.count_nonzero(on & ~kp & (p0 + d > max_v)))
    ev["clip1_q0_lo"] += int(np.count_nonzero(on & ~kq & (q0 - d < 0)))
    ev["clip1_q0_hi"] += int(np.count_nonzero(on & ~kq & (q0 - d > max_v)))
    for v in np.unique((qpl + c_qp_offset)[((ent & BS_MASK) == 2)]):
        ev[("qpi", int(v))] += 1
    return ev


# ---- SAO vectors ------------------------------------------------------------------------------------------------------

def sao_offset_limits(bit_depth):
    """the spec-legal offset magnitudes ((1 << (Min(bitDepth, 10) - 5)) - 1) << log2OffsetScale, log2OffsetScale = 0..
    Max(0, bitDepth - 10), that an int8 SaoOffsetVal holds"""
    base = (1 << (min(bit_depth, 10) - 5)) - 1
    return [base << s for s in range(0, max(0, bit_depth - 10) + 1) if base << s <= 127]


FUSED_COLS, FUSED_ROWS = (63, 64, 191, 192), (127, 128)   # tile and quadrant borders of the fused kernels


def sao_full_range(bit_depth, ctb_log2, rng, *, w=320, h=256, keep_every=6, stripe_cols=FUSED_COLS,
                   stripe_rows=FUSED_ROWS, walk_start=0):
    """Full-range SAO content and parameters for a w x h plane with square CTBs of 1 << ctb_log2:
    8x8 blocks of ramps through all 32 bands, runs of 0 and max_v, plateaus with single-sample spikes (edge categories with
    sgn = 0 next to extremes), full-range noise and 0 / max_v checkers; 0 and max_v side by side across columns 63/64,
    191/192 and rows 127/128 (stripe_cols / stripe_rows: the borders of other kernels; no draw depends on them).  Parameters:
    band CTBs walk every band position 0..31, edge CTBs every class; offsets take the spec-legal scaled magnitudes and the
    int8 ends -128 / 127 (edge offsets signed as 7.4.9.3.2); walk_start: where the walk through the band positions and the
    offset magnitudes begins, for the frames of a plane of few CTBs (the first band CTB takes position 13 * walk_start % 32,
    CTB i the magnitudes of turn i // 5 + walk_start).  Returns plane, params (oracle/h265 SAO_CTB_DTYPE), keep (one byte per
    8x8 block)."""
    max_v = (1 << bit_depth) - 1
    p = np.zeros((h, w), np.int64)
    yy, xx = np.mgrid[0:8, 0:8]
    for by in range(h // 8):
        for bx in range(w // 8):
            kind = int(rng.integers(0, 6))
            if kind == 0:    # ramp: 64 levels over the range, every band hit
                blk = ((xx + 8 * yy) * (max_v + 1)) // 64 + rng.integers(0, max(1, (max_v + 1) // 64), (8, 8))
            elif kind == 1:  # plateau with spikes
                lvl = int(rng.choice([0, max_v, int(rng.integers(0, max_v + 1))]))
                blk = np.full((8, 8), lvl)
                sp = rng.integers(0, 8, (3, 2))
                blk[sp[:, 0], sp[:, 1]] = rng.choice([0, max_v], 3)
            elif kind == 2:  # runs of 0 / max_v
                blk = np.where((xx // int(rng.integers(1, 5)) + yy) % 2 == 0, 0, max_v)
            elif kind == 3:
                blk = rng.integers(0, max_v + 1, (8, 8))
            elif kind == 4:  # low / high bands with small texture
                lvl = int(rng.choice([0, max_v]))
                blk = np.abs(lvl - rng.integers(0, max(2, (max_v + 1) >> 3), (8, 8)))
            else:
                blk = np.where((xx + yy) % 2 == 0, 0, max_v)
            p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = blk
    for c in stripe_cols:
        if c < w:
            p[:, c] = np.where((np.arange(h) + c) % 3 == 0, p[:, c], max_v if c % 2 else 0)
    for r in stripe_rows:
        if r < h:
            p[r] = np.where((np.arange(w) + r) % 3 == 0, p[r], max_v if r % 2 else 0)
    p = np.clip(p, 0, max_v)
    rows, cols = -(-h >> ctb_log2), -(-w >> ctb_log2)
    from oracle import h265
    prm = np.zeros((rows, cols), h265.SAO_CTB_DTYPE)
    lims = sao_offset_limits(bit_depth)
    n_band, n_edge = walk_start, 0
    for i in range(rows * cols):
        r_, c_ = divmod(i, cols)
        t = (0, 1, 2, 1, 2)[i % 5]
        prm["type"][r_, c_] = t
        if t == 1:
            prm["cls"][r_, c_] = (n_band * 13 + i // 32) % 32
            n_band += 1
        elif t == 2:
            prm["cls"][r_, c_] = n_edge % 4
            n_edge += 1
        j = i // 5 + walk_start
        if j % 4 == 3:
            mags = [127, 128, 127, 128]
        else:
            L = lims[j % len(lims)]
            mags = [L, int(rng.integers(0, L + 1)), L, int(rng.integers(0, L + 1))]
        if t == 1:
            off = [min(m, 127) if rng.integers(0, 2) else -m for m in mags]
        else:
            off = [min(mags[0], 127), min(mags[1], 127), -mags[2], -mags[3]]
        prm["offset"][r_, c_] = off
    keep = (rng.integers(0, keep_every, (h // 8, w // 8)) == 0).astype(np.uint8)
    return p.astype(np.uint8 if bit_depth == 8 else np.uint16), prm, keep


def sao_census(plane, params, ctb_log2, bit_depth, keep=None):
    """tags of what SAO does on a plane: ("band", position) where an offset lands, ("wrap", position) for a band below the
    position (29..31), ("edge", class, category), clip_lo / clip_hi, ("offset", value) of an applied offset"""
    src = np.asarray(plane, np.int64)
    h, w = src.shape
    max_v = (1 << bit_depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    P = np.asarray(params).ravel()
    ci = (yy >> ctb_log2) * np.asarray(params).shape[1] + (xx >> ctb_log2)
    typ, cls = P["type"].astype(np.int64)[ci], P["cls"].astype(np.int64)[ci]
    offs = P["offset"].astype(np.int64)
    live = np.ones((h, w), bool) if keep is None else np.asarray(keep)[yy >> 3, xx >> 3] == 0
    tags = set()
    band = src >> (bit_depth - 5)
    k = (band - cls) & 31
    bsel = live & (typ == 1) & (k < 4)
    for pos in np.unique(cls[bsel]):
        tags.add(("band", int(pos)))
    for pos in np.unique(cls[bsel & (band < cls)]):
        tags.add(("wrap", int(pos)))
    pad = np.pad(src, 1, constant_values=-1)
    inside = np.pad(np.ones((h, w), bool), 1, constant_values=False)
    hv = {0: ((0, -1), (0, 1)), 1: ((-1, 0), (1, 0)), 2: ((-1, -1), (1, 1)), 3: ((-1, 1), (1, -1))}
    idx = np.where(bsel, k + 1, 0)
    for c, ((ay, ax), (by_, bx_)) in hv.items():
        a = pad[1 + ay:1 + ay + h, 1 + ax:1 + ax + w]
        b = pad[1 + by_:1 + by_ + h, 1 + bx_:1 + bx_ + w]
        ok = inside[1 + ay:1 + ay + h, 1 + ax:1 + ax + w] & inside[1 + by_:1 + by_ + h, 1 + bx_:1 + bx_ + w]
        e = 2 + np.sign(src - a) + np.sign(src - b)
        e = np.where(e <= 2, np.where(e == 2, 0, e + 1), e)
        sel = live & (typ == 2) & (cls == c) & ok & (e > 0)
        for cat in np.unique(e[sel]):
            tags.add(("edge", c, int(cat)))
        idx = np.where(sel, e, idx)
    applied = idx > 0
    val = np.where(applied, offs[ci, np.maximum(idx - 1, 0)], 0)
    if (applied & (src + val < 0)).any():
        tags.add("clip_lo")
    if (applied & (src + val > max_v)).any():
        tags.add("clip_hi")
    for v in np.unique(val[applied]):
        tags.add(("offset", int(v)))
    return tags
