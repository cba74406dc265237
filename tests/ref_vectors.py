"""Test vectors for the reference-exact mode at its decision edges, and an independent numpy restatement of that filter.

TEST INFRASTRUCTURE ONLY.  The reference-exact mode is the filter of the reference's CPU header (cpu.h) with its quirks
(SURVEY Q-list).  Two things live here:

* reference_plane(): cpu.h's block loop (cpu.h:134-992), luma segment (CheckLocalAdaptivity / IsStrongFilterToUse /
  ApplyStrongFilter / ApplyNormalFilter, cpu.h:1074-1429) and chroma segment (cpu.h:1431-1488) restated in numpy int64 from
  the reference's text.  It shares nothing with oracle/deblock_oracle_impl.inc but the two tables.  Offset blocks are
  independent, so it runs ver1 -> ver2 -> hor1 -> hor2 on all blocks at once.  Besides the filtered plane
  it reports what every segment did: a label, which clips fired and which thresholds were met exactly at value - 1 and at
  value, measured at decision time on the samples as they then are.
* constructive generators: luma planes whose segments are solved onto each decision threshold of the reference, onto the
  range extremes and onto the picture border (luma_plane), chroma planes on the +-tc clips and Clip2 (chroma_plane), the
  operand sets that go with them (custom tables, the packed core's operand-range edge, QP maps) and whole 8-bit 4:2:0 frames (boundary_frame).

Everything is generated from a numpy Generator, so a test needs no stored vectors.
"""
from collections import Counter

import numpy as np

from h265_vectors import _line, _sgn, _split

# cpu.h:1021-1033
BETA_TABLE = np.array([0] * 16 + [6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42,
                       44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64], np.int64)
TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20], np.int64)
assert BETA_TABLE.size == 52 and TC_TABLE.size == 52

SEGS = ("ver1", "ver2", "hor1", "hor2")
LABELS = ("off", "strong", "normal_p0q0", "normal_p0q1", "normal_p1q0", "normal_p1q1", "normal_skipped", "chroma")
NOT_FILTERED = -1  # label of a segment whose bS does not enable it
LUMA_CLIPS = tuple("strong_%s_%s" % (t, e) for t in ("p0", "p1", "p2", "q0", "q1", "q2") for e in ("lo", "hi")) + \
    tuple("%s_%s" % (t, e) for t in ("delta", "dp1", "dq1") for e in ("lo", "hi")) + \
    tuple("clip2_%s_%s" % (t, e) for t in ("p0", "p1", "q0", "q1") for e in ("lo", "hi"))
CHROMA_CLIPS = ("cdp_lo", "cdp_hi", "cdq_lo", "cdq_hi", "cclip2_p0_lo", "cclip2_p0_hi", "cclip2_q0_lo", "cclip2_q0_hi")
LUMA_THRESHOLDS = ("d", "dpq0", "dpq3", "e0", "e3", "f0", "f3", "side_p", "side_q", "delta")
CHROMA_THRESHOLDS = ("dp", "dq")
BORDERS = ("left", "right", "top", "bottom")


def _tap_rc(seg):
    """(row, col) inside the 8x8 offset block of P_k / Q_k of line i: arrays [k][i] (cpu.h:159-446)"""
    k, i = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    if seg == 0:    # ver1: line i = row i, P_k = col 3-k, Q_k = col 4+k
        return (i, 3 - k), (i, 4 + k)
    if seg == 1:    # ver2: rows 4..7
        return (4 + i, 3 - k), (4 + i, 4 + k)
    if seg == 2:    # hor1: line i = col i, P_k = row 3-k, Q_k = row 4+k
        return (3 - k, i), (4 + k, i)
    return (3 - k, 4 + i), (4 + k, i)   # hor2: P line i = col 4+i, Q line i = col i


TAPS = [_tap_rc(s) for s in range(4)]
# P0 / Q0 of line 0 of each segment, offsets from the block's top-left image position (x0, y0) = (8bx - 4, 8by - 4)
QP_POS = (((3, 0), (4, 0)), ((3, 4), (4, 4)), ((0, 3), (0, 4)), ((4, 3), (0, 4)))


def tables_of(tc_table=None, beta_table=None):
    tc = TC_TABLE if tc_table is None else np.asarray(tc_table, np.int64)
    beta = BETA_TABLE if beta_table is None else np.asarray(beta_table, np.int64)
    assert tc.size == 52 and beta.size == 52
    return tc, beta


def seg_operands(seg, bx, by, *, w, h, is_chroma=False, bit_depth=8, qp=30, qp_map=None, ctu_log2=6, tc_table=None,
                 beta_table=None):
    """(beta, tc) of segment `seg` of offset block(s) (bx, by) of a w x h plane (arrays broadcast): the table entries of the
    scalar QP (cpu.h:136-137, 1064-1072), or of (QpP + QpQ + 1) >> 1, then min(., 51), where QpP / QpQ are the map entries at
    P0 / Q0 of the segment's line 0 (luma coordinates, clamped into the picture), scaled by 1 << (bit_depth - 8)"""
    tc_t, beta_t = tables_of(tc_table, beta_table)
    bx, by = np.asarray(bx, np.int64), np.asarray(by, np.int64)
    if qp_map is None:
        q = np.full(np.broadcast(bx, by).shape, min(int(qp), 51), np.int64)
    else:
        m = np.asarray(qp_map, np.int64)
        sc = 2 if is_chroma else 1
        x0, y0 = 8 * bx - 4, 8 * by - 4

        def at(dx, dy):
            lx = np.clip((x0 + dx) * sc, 0, w * sc - 1)
            ly = np.clip((y0 + dy) * sc, 0, h * sc - 1)
            return m[ly >> ctu_log2, lx >> ctu_log2]
        (pxo, pyo), (qxo, qyo) = QP_POS[seg]
        q = np.minimum((at(pxo, pyo) + at(qxo, qyo) + 1) >> 1, 51)
    sh = bit_depth - 8
    return beta_t[q] << sh, tc_t[q] << sh


def segment_coords(seg, bx, by):
    """image (y, x) of the taps p3 p2 p1 p0 q0 q1 q2 q3 of the four lines of a segment: two (4, 8) arrays"""
    (pr, pc), (qr, qc) = TAPS[seg]
    r = np.concatenate([pr[::-1].T, qr.T], axis=1)
    c = np.concatenate([pc[::-1].T, qc.T], axis=1)
    return 8 * by - 4 + r, 8 * bx - 4 + c


def new_stats():
    return {"labels": Counter(), "clips": Counter(), "events": Counter(), "extras": Counter()}


def merge_stats(a, b):
    for k in a:
        a[k].update(b[k])
    return a


def _ev(st, name, x, t, where):
    """x < t met exactly: at value - 1 (x == t - 1, passes) and at value (x == t, fails)"""
    st["events"][(name, "below")] += int(np.count_nonzero(where & (x == t - 1)))
    st["events"][(name, "at")] += int(np.count_nonzero(where & (x == t)))


def _luma_segment(P, Q, on, beta, tc, max_v, st):
    """cpu.h:1359-1429 on every block at once.  P[k] / Q[k]: (nby, nbx, 4 lines); beta, tc: (nby, nbx).  Returns the new
    P, Q, the labels and the per-line normal-filter numerators."""
    p0, p1, p2, p3 = P
    q0, q1, q2, q3 = Q
    T = tc[..., None]
    dp = np.abs(p2 - 2 * p1 + p0)
    dq = np.abs(q2 - 2 * q1 + q0)
    dp0, dp3, dq0, dq3 = dp[..., 0], dp[..., 3], dq[..., 0], dq[..., 3]
    # condition (1), cpu.h:1086-1087: lines 0 and 3 only
    d = dp0 + dp3 + dq0 + dq3
    filt = on & (d < beta)
    # conditions (2)-(4), cpu.h:1099-1110: beta / 8 and 5 * tc / 2 truncate
    b8, t52 = beta // 8, (5 * tc) // 2
    dpq = {0: dp0 + dq0, 3: dp3 + dq3}
    e = {i: np.abs(p3[..., i] - p0[..., i]) + np.abs(q0[..., i] - q3[..., i]) for i in (0, 3)}
    f = {i: np.abs(p0[..., i] - q0[..., i]) for i in (0, 3)}
    c2 = {i: dpq[i] < b8 for i in (0, 3)}
    c3 = {i: e[i] < b8 for i in (0, 3)}
    c4 = {i: f[i] < t52 for i in (0, 3)}
    strong = filt & c2[0] & c2[3] & c3[0] & c3[3] & c4[0] & c4[3]
    normal = filt & ~strong
    # cond5 / cond6, cpu.h:1243-1249: 3 * beta / 16 truncates
    side = (3 * beta) // 16
    cond5, cond6 = (dp0 + dp3) < side, (dq0 + dq3) < side
    _ev(st, "d", d, beta, on)
    for i, j in ((0, 3), (3, 0)):   # decisive: every other condition of the strong decision holds
        rest = filt & c2[j] & c3[j] & c4[j]
        _ev(st, "dpq%d" % i, dpq[i], b8, rest & c3[i] & c4[i])
        _ev(st, "e%d" % i, e[i], b8, rest & c2[i] & c4[i])
        _ev(st, "f%d" % i, f[i], t52, rest & c2[i] & c3[i])
    _ev(st, "side_p", dp0 + dp3, side, normal)
    _ev(st, "side_q", dq0 + dq3, side, normal)

    # ApplyStrongFilter, cpu.h:1152-1211: deltas clipped at c = 2 * tc, then Clip2
    c = 2 * T
    S = strong[..., None]
    raw = {"p0": (p2 + 2 * p1 - 6 * p0 + 2 * q0 + q1 + 4) >> 3, "p1": (p2 - 3 * p1 + p0 + q0 + 2) >> 2,
           "p2": (2 * p3 - 5 * p2 + p1 + p0 + q0 + 4) >> 3, "q0": (q2 + 2 * q1 - 6 * q0 + 2 * p0 + p1 + 4) >> 3,
           "q1": (q2 - 3 * q1 + q0 + p0 + 2) >> 2, "q2": (2 * q3 - 5 * q2 + q1 + q0 + p0 + 4) >> 3}
    orig = {"p0": p0, "p1": p1, "p2": p2, "q0": q0, "q1": q1, "q2": q2}
    new = dict(orig)
    for k, r in raw.items():
        st["clips"]["strong_%s_lo" % k] += int(np.count_nonzero(S & (r < -c)))
        st["clips"]["strong_%s_hi" % k] += int(np.count_nonzero(S & (r > c)))
        new[k] = np.where(S, np.clip(orig[k] + np.clip(r, -c, c), 0, max_v), new[k])
    st["extras"]["strong_sum_max"] += int(np.count_nonzero(S & (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 == 8 * max_v)))

    # ApplyNormalFilter, cpu.h:1233-1354: per line |delta| < 10 tc; clip(delta, 2 tc), tc / 2 for p1 / q1
    N = normal[..., None]
    num = 9 * (q0 - p0) - 3 * (q1 - p1) + 8
    delta = num >> 4
    _ev(st, "delta", np.abs(delta), 10 * T, N)
    apply = N & (np.abs(delta) < 10 * T)
    D = np.clip(delta, -c, c)
    h = T // 2
    rp1 = (((p2 + p0 + 1) >> 1) - p1 + D) >> 1
    rq1 = (((q2 + q0 + 1) >> 1) - q1 - D) >> 1
    m5, m6 = apply & cond5[..., None], apply & cond6[..., None]
    cnt = st["clips"]
    cnt["delta_lo"] += int(np.count_nonzero(apply & (delta < -c)))
    cnt["delta_hi"] += int(np.count_nonzero(apply & (delta > c)))
    cnt["dp1_lo"] += int(np.count_nonzero(m5 & (rp1 < -h)))
    cnt["dp1_hi"] += int(np.count_nonzero(m5 & (rp1 > h)))
    cnt["dq1_lo"] += int(np.count_nonzero(m6 & (rq1 < -h)))
    cnt["dq1_hi"] += int(np.count_nonzero(m6 & (rq1 > h)))
    cand = {"p0": (p0 + D, apply), "q0": (q0 - D, apply), "p1": (p1 + np.clip(rp1, -h, h), m5), "q1": (q1 + np.clip(rq1, -h, h), m6)}
    for k, (v, g) in cand.items():
        cnt["clip2_%s_lo" % k] += int(np.count_nonzero(g & (v < 0)))
        cnt["clip2_%s_hi" % k] += int(np.count_nonzero(g & (v > max_v)))
        new[k] = np.where(g, np.clip(v, 0, max_v), new[k])
    skipped = normal & ~apply.any(axis=-1)
    lab = np.where(~on, NOT_FILTERED, np.where(~filt, 0, np.where(strong, 1, np.where(skipped, 6, 2 + 2 * cond5 + cond6))))
    return [new["p0"], new["p1"], new["p2"], p3], [new["q0"], new["q1"], new["q2"], q3], lab, np.where(apply, num, 0)


def _chroma_segment(P, Q, on, tc, max_v, st):
    """cpu.h:1431-1488: the P delta from (p0 - q0), the Q delta from (q0 - p0) and subtracted; tc, no beta"""
    p0, p1 = P[0], P[1]
    q0, q1 = Q[0], Q[1]
    T = tc[..., None]
    O = np.broadcast_to(on[..., None], p0.shape)
    dp = ((p0 - q0) * 4 + p1 - q1 + 4) >> 3
    dq = ((q0 - p0) * 4 + q1 - p1 + 4) >> 3
    # the clip of each delta at +-tc: |delta| == tc passes untouched, |delta| == tc + 1 is clipped
    _ev(st, "dp", np.abs(dp), T + 1, O)
    _ev(st, "dq", np.abs(dq), T + 1, O)
    cnt = st["clips"]
    cnt["cdp_lo"] += int(np.count_nonzero(O & (dp < -T)))
    cnt["cdp_hi"] += int(np.count_nonzero(O & (dp > T)))
    cnt["cdq_lo"] += int(np.count_nonzero(O & (dq < -T)))
    cnt["cdq_hi"] += int(np.count_nonzero(O & (dq > T)))
    st["extras"]["chroma_round"] += int(np.count_nonzero(O & (dp != -dq)))
    np0 = p0 + np.clip(dp, -T, T)
    nq0 = q0 - np.clip(dq, -T, T)
    for k, v in (("p0", np0), ("q0", nq0)):
        cnt["cclip2_%s_lo" % k] += int(np.count_nonzero(O & (v < 0)))
        cnt["cclip2_%s_hi" % k] += int(np.count_nonzero(O & (v > max_v)))
    P = [np.where(O, np.clip(np0, 0, max_v), p0)] + list(P[1:])
    Q = [np.where(O, np.clip(nq0, 0, max_v), q0)] + list(Q[1:])
    return P, Q, np.where(on, 7, NOT_FILTERED)


def reference_plane(plane, qp, *, is_chroma=False, bit_depth=8, vert_bs=None, hor_bs=None, qp_map=None, ctu_log2=6,
                    tc_table=None, beta_table=None, stats=None):
    """cpu.h:134-992 on one un-padded plane (H x W, multiples of 8).  vert_bs / hor_bs in the reference's layouts (None = the
    default pattern of cpu.h:92-99 / 110-117).  Returns (filtered plane, info): info["labels"] is (nby, nbx, 4) -- the label
    of ver1, ver2, hor1, hor2 of each offset block (index into LABELS, NOT_FILTERED where bS leaves the segment alone),
    info["stats"] counts labels, clips, threshold events ((name, "below" | "at")) and extras (border segments, hor2)."""
    src = np.asarray(plane)
    H, W = src.shape
    st = new_stats() if stats is None else stats
    max_v = (1 << bit_depth) - 1
    # zero padding of 4 samples (cpu.h:55-71); offset block (bx, by) = padded rows 8by.., cols 8bx..
    pad = np.zeros((H + 8, W + 8), np.int64)
    pad[4:H + 4, 4:W + 4] = src
    nbx, nby = W // 8 + 1, H // 8 + 1
    blk = np.ascontiguousarray(pad.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3))
    vs, hs = W // 8 + 1, W // 8
    n_vert, n_hor = vs * (H // 8), (H // 8 + 1) * hs
    if vert_bs is None:
        i = np.arange(n_vert)
        vert_bs = np.where(i % vs == 0, 0, 2)
    if hor_bs is None:
        i = np.arange(n_hor)
        hor_bs = np.where(i % (H // 8 + 1) == 0, 0, 2)   # the zeroing stride H/8 + 1
    vb, hb = np.asarray(vert_bs, np.int64).ravel(), np.asarray(hor_bs, np.int64).ravel()
    assert vb.size == n_vert and hb.size == n_hor
    # the ver2 / hor2 guards: the plane's own block counts for luma, the LUMA plane's for chroma
    lim_x = 2 * W // 8 if is_chroma else nbx - 1
    lim_y = 2 * H // 8 if is_chroma else nby - 1
    BY, BX = np.meshgrid(np.arange(nby), np.arange(nbx), indexing="ij")

    def bs_at(arr, ok, idx):
        ok = ok & (idx >= 0) & (idx < arr.size)   # reads past the end act on padding only: skipped
        return np.where(ok, arr[np.clip(idx, 0, max(arr.size - 1, 0))] if arr.size else 0, 0)
    bss = (bs_at(vb, BY > 0, (BY - 1) * vs + BX), bs_at(vb, BY < lim_y, BY * vs + BX),
           bs_at(hb, BX > 0, BY * hs + BX - 1), bs_at(hb, BX < lim_x, BY * hs + BX))
    labels = np.full((nby, nbx, 4), NOT_FILTERED, np.int64)
    ops = dict(w=W, h=H, is_chroma=is_chroma, bit_depth=bit_depth, qp=qp, qp_map=qp_map, ctu_log2=ctu_log2,
               tc_table=tc_table, beta_table=beta_table)
    for s in range(4):
        (pr, pc), (qr, qc) = TAPS[s]
        P = [blk[:, :, pr[k], pc[k]] for k in range(4)]
        Q = [blk[:, :, qr[k], qc[k]] for k in range(4)]
        beta, tc = seg_operands(s, BX, BY, **ops)
        bs = bss[s]
        if is_chroma:
            on = bs == 2                       # cpu.h:463, 519, 572, 649
            P, Q, lab = _chroma_segment(P, Q, on, tc, max_v, st)
            live = on
        else:
            on = bs > 0                        # cpu.h:164, 228, 292, 373 (bS 1 == bS 2 for luma)
            P, Q, lab, num = _luma_segment(P, Q, on, beta, tc, max_v, st)
            live = lab > 0
            top = 6 * max_v + 6 * (max_v // 3) + 8   # the largest legal numerator (p = 0, a, 2a, 3a | q = M, M - a, ..)
            st["extras"]["max_ramp"] += int(np.count_nonzero(np.abs(num - 8) == top - 8))
        for k in range(4):
            blk[:, :, pr[k], pc[k]] = P[k]
            blk[:, :, qr[k], qc[k]] = Q[k]
        labels[:, :, s] = lab
        for i, name in enumerate(LABELS):
            st["labels"][name] += int(np.count_nonzero(lab == i))
        # segments with one side wholly in the zero padding, filtered against it
        ys, xs = 8 * BY[..., None, None] - 4, 8 * BX[..., None, None] - 4
        inside = lambda r, c: (ys + r >= 0) & (ys + r < H) & (xs + c >= 0) & (xs + c < W)
        p_out = ~inside(pr, pc).any(axis=(-2, -1))
        q_out = ~inside(qr, qc).any(axis=(-2, -1))
        edge = live & (p_out ^ q_out)
        if s < 2:
            st["extras"]["border_left"] += int(np.count_nonzero(edge & (BX == 0)))
            st["extras"]["border_right"] += int(np.count_nonzero(edge & (BX == nbx - 1)))
        else:
            st["extras"]["border_top"] += int(np.count_nonzero(edge & (BY == 0)))
            st["extras"]["border_bottom"] += int(np.count_nonzero(edge & (BY == nby - 1)))
            if s == 3:
                st["extras"]["hor2"] += int(np.count_nonzero(live))
                st["extras"]["hor2_q_padding"] += int(np.count_nonzero(edge & (BX == 0)))
        if is_chroma:
            st["extras"]["chroma_shifted_read"] += int(np.count_nonzero(live & (BX == nbx - 1) & (s == 3)))
    out = blk.transpose(0, 2, 1, 3).reshape(H + 8, W + 8)[4:H + 4, 4:W + 4]
    return out.astype(src.dtype), {"labels": labels, "stats": st}


# ---- luma vectors -----------------------------------------------------------------------------------------------------

class LumaBuilder:
    """solves one segment's 4 x 8 samples (lines x p3..q3) onto a case; counters alternate the threshold side and line"""

    CASES = ("d", "dpq", "e", "f", "side", "delta", "step", "clip2", "strongclip", "maxramp", "extreme", "texture")
    BORDER_CASES = ("bf", "bd", "bdelta", "bmax", "btexture")   # one side wholly zero padding

    def __init__(self, rng, bit_depth):
        self.rng, self.bd = rng, bit_depth
        self.max_v = (1 << bit_depth) - 1
        self.n = Counter()

    def _side(self, name):
        self.n[name] += 1
        return self.n[name] % 2   # 0: value - 1, 1: value

    def _small_g(self, t52):
        return int(self.rng.integers(-(t52 - 1), t52)) if t52 > 1 else 0

    def _which(self, name, ln, other):
        self.n[name + "_line"] += 1
        return [ln, other] if (self.n[name + "_line"] // 2) % 2 else [other, ln]

    def _place(self, lines, flip=True):
        """lines 0 and 3 -> an absolute 4 x 8 segment at a random level; lines 1 and 2 (which no decision reads)
        copy them or carry extra texture"""
        r = self.rng
        seg = np.array([lines[0], lines[0], lines[1], lines[1]], np.int64)
        if r.integers(0, 2):
            seg[1:3] += r.integers(-3, 4, (2, 8)) * (1 + int(r.integers(0, 8)))
        lo, hi = seg.min(), seg.max()
        if hi - lo > self.max_v:
            return None
        seg = seg + int(r.integers(0, self.max_v - (hi - lo) + 1)) - lo
        if flip and r.integers(0, 2):
            seg = self.max_v - seg
        if flip and r.integers(0, 2):
            seg = seg[:, ::-1]
        return seg

    def build(self, case, beta, tc):
        r = self.rng
        b8, t52, side = beta // 8, (5 * tc) // 2, (3 * beta) // 16
        flat = lambda: _line(0, self._small_g(t52))
        if case == "d":
            if beta < 1:
                return None
            parts = _split(r, beta - 1 + self._side("d"), 4)
            ls = []
            for k in (0, 2):
                cp, cq = parts[k] * _sgn(r), parts[k + 1] * _sgn(r)
                ls.append(_line(0, self._small_g(t52), cp=cp, ep=-cp, cq=cq, eq=-cq))
            return self._place(ls)
        if case == "dpq":   # dp_i + dq_i < beta / 8 on one line, everything else of the strong decision held
            if b8 < 1:
                return None
            a, b = _split(r, b8 - 1 + self._side("dpq"), 2)
            cp, cq = a * _sgn(r), b * _sgn(r)
            return self._place(self._which("dpq", _line(0, self._small_g(t52), cp=cp, ep=-cp, cq=cq, eq=-cq), flat()))
        if case == "e":
            if b8 < 1:
                return None
            a, b = _split(r, b8 - 1 + self._side("e"), 2)
            return self._place(self._which("e", _line(0, self._small_g(t52), ep=a * _sgn(r), eq=b * _sgn(r)), flat()))
        if case == "f":
            if t52 < 1:
                return None
            x = t52 - 1 + self._side("f")
            return self._place(self._which("f", _line(0, x * _sgn(r)), flat()))
        if case == "side":   # cond5 / cond6 of the normal filter; |p0 - q0| >= 5 tc / 2 keeps the strong filter off
            if side < 1:
                return None
            xp = side - 1 + self._side("side")
            xq = [side - 1, side, 0, int(r.integers(0, side + 1))][self.n["side_q"] % 4]
            self.n["side_q"] += 1
            (ap, bp), (aq, bq) = _split(r, xp, 2), _split(r, xq, 2)
            ls = []
            for cp, cq in ((ap, aq), (bp, bq)):
                cp, cq = cp * _sgn(r), cq * _sgn(r)
                g = max(t52, 1) + int(r.integers(0, max(t52, 1) + 1))
                ls.append(_line(0, g * _sgn(r), cp=cp, ep=-cp, cq=cq, eq=-cq))
            return self._place(ls)
        if case == "delta":   # |delta| against 10 tc: numerator 9 (q0 - p0) - 3 (q1 - p1) + 8 solved into [16 K, 16 K + 15]
            K = 10 * tc - 1 + self._side("delta")
            if K < 1 or beta < 1:
                return None
            mirror, swap = bool(r.integers(0, 2)), bool(r.integers(0, 2))
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
                ln = np.array(_line(int(r.integers(amin, amax + 1)), g, sp=a, sq=-b), np.int64)
                seg = np.array([ln] * 4)
                if mirror:
                    seg = self.max_v - seg
                return seg[:, ::-1] if swap else seg
            return None
        if case == "step":   # a plain step: |delta| between 2 tc and 10 tc -> clip(delta, 2 tc) and the tc / 2 clips
            if tc < 1 or beta < 1:
                return None
            glo, ghi = (2 * tc * 16) // 9 + 2, (10 * tc * 16 - 8) // 9 - 1
            ghi = min(ghi, self.max_v)
            if glo > ghi:
                return None
            g = int(r.integers(glo, ghi + 1))
            return self._place([_line(0, g), _line(0, g)])
        if case == "clip2":   # p0 at the bottom of the range, the Q side rising: p0 + D leaves [0, max_v]
            if tc < 1 or beta < 1:
                return None
            c = int(r.integers(0, 2 * tc))
            q0 = int(r.integers(0, c + 1))
            smin = max(2 * tc, b8 // 3 + 1, 1)
            smax = min((self.max_v - q0) // 3, 50 * tc)
            if smin > smax:
                return None
            s = int(r.integers(smin, smax + 1))
            ln = np.array([c, c, c, c, q0, q0 + s, q0 + 2 * s, q0 + 3 * s], np.int64)
            seg = np.array([ln] * 4)
            if r.integers(0, 2):
                seg = self.max_v - seg
            return seg[:, ::-1] if r.integers(0, 2) else seg
        if case == "strongclip":
            return self._strong_clip(beta, tc)
        if case == "maxramp":
            a = self.max_v // 3
            seg = np.array([_line(0, self.max_v, sp=a, sq=-a)] * 4, np.int64)
            return seg[:, ::-1] if r.integers(0, 2) else seg
        if case == "extreme":
            k = self.n["extreme"] % 3
            self.n["extreme"] += 1
            if k == 0:
                return np.full((4, 8), self.max_v, np.int64)
            if k == 1:
                return np.zeros((4, 8), np.int64)
            seg = np.array([[0] * 4 + [self.max_v] * 4] * 4, np.int64)
            return seg[:, ::-1] if r.integers(0, 2) else seg
        g = int(r.integers(-4 * max(tc, 1), 4 * max(tc, 1) + 1))
        seg = np.array([[0] * 4 + [g] * 4] * 4, np.int64) + (r.integers(-6, 7, (4, 8)) << (self.bd - 8))
        return self._place([seg[0], seg[3]])

    def _strong_clip(self, beta, tc):
        """strong-filter content (every condition of IsStrongFilterToUse just met) whose deltas leave +-2 tc: random search"""
        r = self.rng
        b8, t52 = beta // 8, (5 * tc) // 2
        td, te, tf = b8 - 1, b8 - 1, t52 - 1
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
        ep = ea * np.where(r.integers(0, 2, n) > 0, 1, -1) - 3 * sp - cp
        eq = eb * np.where(r.integers(0, 2, n) > 0, 1, -1) - 3 * sq - cq
        g = r.integers(-tf, tf + 1, n)
        L = np.array(_line(np.zeros(n, np.int64), g, sp, cp, ep, sq, cq, eq))
        p3, p2, p1, p0, q0, q1, q2, q3 = L
        outs = [(p2 + 2 * p1 - 6 * p0 + 2 * q0 + q1 + 4) >> 3, (p2 - 3 * p1 + p0 + q0 + 2) >> 2,
                (2 * p3 - 5 * p2 + p1 + p0 + q0 + 4) >> 3]
        k = self.n["strongclip"] % 12
        self.n["strongclip"] += 1
        o = np.asarray(outs[(k // 2) % 3])
        hit = np.nonzero(o < -2 * tc if k % 2 == 0 else o > 2 * tc)[0]
        if not hit.size:
            hit = np.nonzero(np.max(np.abs(np.array(outs)), axis=0) > 2 * tc)[0]
            if not hit.size:
                return None
        seg = np.array([L[:, hit[0]]] * 4, np.int64)
        if k >= 6:   # the filter is symmetric under p <-> q: the Q-side targets are the P-side ones, reversed
            seg = seg[:, ::-1]
        lo, hi = seg.min(), seg.max()
        if hi - lo > self.max_v:
            return None
        return seg + int(r.integers(0, self.max_v - (hi - lo) + 1)) - lo

    def build_border(self, case, beta, tc):
        """a segment whose P side is the zero padding (the caller reverses it for a Q side in the padding)"""
        r = self.rng
        t52 = (5 * tc) // 2
        q = None
        if case == "bf":      # Q flat: |p0 - q0| = q0 against 5 tc / 2, everything else 0
            x = max(t52 - 1 + self._side("bf"), 0)
            q = np.full((4, 4), x, np.int64)
        elif case == "bd":    # Q curvature on lines 0 and 3: d against beta
            if beta < 1:
                return None
            c0, c3 = _split(r, beta - 1 + self._side("bd"), 2)
            q = np.zeros((4, 4), np.int64)
            q[0, 0], q[3, 0] = c0, c3
            q[1:3] = r.integers(0, 3, (2, 4))
        elif case == "bdelta":   # Q flat at g: delta = (6 g + 8) >> 4 against 10 tc
            K = 10 * tc - 1 + self._side("bdelta")
            if K < 1 or beta < 1:
                return None
            g = -((-(16 * K - 8)) // 6)
            if g > self.max_v:
                return None
            q = np.full((4, 4), g, np.int64)
        elif case == "bmax":
            q = np.full((4, 4), self.max_v, np.int64)
        else:
            q = r.integers(0, self.max_v + 1, (4, 4))
        if q.max() > self.max_v:
            return None
        return np.concatenate([np.zeros((4, 4), np.int64), q], axis=1)


WAVES = ("v", "h", "mixed")


def _put(plane, seg_kind, bx, by, seg):
    """write a solved segment's in-picture taps"""
    H, W = plane.shape
    ys, xs = segment_coords(seg_kind, bx, by)
    m = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    plane[ys[m], xs[m]] = seg[m]


def _solve(bld, plane, seg_kind, bx, by, ops, border, k):
    """solve segment (seg_kind, bx, by) of the plane onto the next case; returns the next case counter"""
    H, W = plane.shape
    ys, xs = segment_coords(seg_kind, bx, by)
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    p_in, q_in = inside[:, :4].any(), inside[:, 4:].any()
    if not p_in and not q_in:
        return k
    beta, tc = (int(v) for v in seg_operands(seg_kind, bx, by, w=W, h=H, **ops))
    seg = None
    cases = LumaBuilder.CASES if p_in and q_in else LumaBuilder.BORDER_CASES
    if not (p_in and q_in) and not border:
        return k
    for _ in range(len(cases)):
        case = cases[k % len(cases)]
        k += 1
        seg = bld.build(case, beta, tc) if p_in and q_in else bld.build_border(case, beta, tc)
        if seg is not None:
            break
    if seg is None:
        seg = bld.build("texture", beta, tc) if p_in and q_in else bld.build_border("btexture", beta, tc)
    if not q_in:   # the filter is symmetric under p <-> q
        seg = seg[:, ::-1]
    assert seg.min() >= 0 and seg.max() <= bld.max_v
    _put(plane, seg_kind, bx, by, seg)
    return k


def luma_plane(bit_depth, rng, *, w=528, h=32, wave="v", border=True, qp=30, qp_map=None, ctu_log2=6, tc_table=None,
               beta_table=None):
    """A w x h luma plane (multiples of 8) with its bS arrays (reference layouts) whose enabled segments are each solved for a
    case of LumaBuilder, with (beta, tc) of that segment.
      wave "v": vertical edges only (hor bS 0); each vert entry enables ver2 of one block and ver1 of the block below, the
                four segments' taps are disjoint, so every label holds as solved.  Picture-border entries (x = 0, x = W) are
                filtered against the zero padding when border is set.
      wave "h": horizontal edges only; entries of even columns c enable hor2 of block c -- P taps in columns 4..7 above the
                edge, Q taps in columns 0..3 below it -- and hor1 of block c + 1; odd columns stay 0, so hor1 and
                hor2 of one block never share their Q taps.  Rows y = 0 / y = H are the top / bottom border.
      wave "mixed": both on top of each other and bS 0 / 1 / 2 drawn everywhere: only the measured census holds.
    Returns plane, vert_bs, hor_bs."""
    assert w % 8 == 0 and h % 8 == 0
    max_v = (1 << bit_depth) - 1
    plane = rng.integers(max_v // 4, 3 * max_v // 4 + 1, (h, w)).astype(np.int64)
    vs, hs = w // 8 + 1, w // 8
    vb = np.zeros((h // 8, vs), np.uint8)
    hb = np.zeros((h // 8 + 1, hs), np.uint8)
    ops = dict(bit_depth=bit_depth, qp=qp, qp_map=qp_map, ctu_log2=ctu_log2, tc_table=tc_table, beta_table=beta_table)
    bld = LumaBuilder(rng, bit_depth)
    k = int(rng.integers(0, 64))

    def bs_draw():
        return 0 if rng.integers(0, 8) == 0 else int(rng.integers(1, 3))
    if wave in ("v", "mixed"):
        for r in range(h // 8):
            for bx in range(vs):
                if not border and bx in (0, vs - 1):
                    continue
                vb[r, bx] = bs_draw()
                k = _solve(bld, plane, 1, bx, r, ops, border, k)       # ver2 of block (bx, r): rows 8r .. 8r+3
                k = _solve(bld, plane, 0, bx, r + 1, ops, border, k)   # ver1 of block (bx, r+1): rows 8r+4 .. 8r+7
    if wave in ("h", "mixed"):
        for by in range(h // 8 + 1):
            if not border and by in (0, h // 8):
                continue
            for c in range(0, hs, 2):
                hb[by, c] = bs_draw()
                k = _solve(bld, plane, 3, c, by, ops, border, k)       # hor2 of block c
                if c + 1 <= hs:
                    k = _solve(bld, plane, 2, c + 1, by, ops, border, k)   # hor1 of block c + 1
    if wave == "mixed":
        vb = rng.integers(0, 3, vb.shape).astype(np.uint8)
        hb = rng.integers(0, 3, hb.shape).astype(np.uint8)
    return plane.astype(np.uint8 if bit_depth == 8 else np.uint16), vb.ravel(), hb.ravel()


# ---- chroma vectors ---------------------------------------------------------------------------------------------------

class ChromaBuilder:
    """one chroma segment (4 lines x p3..q3; only p1 p0 q0 q1 are read) onto the +-tc clips of dp and of dq separately, the
    rounding cases x = 4 (p0 - q0) + p1 - q1 == 4 (mod 8) where dp != -dq, and Clip2 at 0 / max_v"""

    CASES = ("dp", "dq", "round", "clip2", "extreme", "small")

    def __init__(self, rng, bit_depth):
        self.rng, self.bd = rng, bit_depth
        self.max_v = (1 << bit_depth) - 1
        self.n = Counter()

    def _line_for(self, x):
        """p1 p0 | q0 q1 with 4 (p0 - q0) + (p1 - q1) == x, at random levels (None if it does not fit)"""
        r = self.rng
        b = int(x % 4) + 4 * int(r.integers(-1, 2))
        a = (x - b) // 4
        lo0, hi0 = max(0, -a), min(self.max_v, self.max_v - a)
        lo1, hi1 = max(0, -b), min(self.max_v, self.max_v - b)
        if lo0 > hi0 or lo1 > hi1:
            return None
        q0, q1 = int(r.integers(lo0, hi0 + 1)), int(r.integers(lo1, hi1 + 1))
        return [q0 + a, q0, q1 + b, q1]   # p0, q0, p1, q1

    def build(self, case, tc):
        r = self.rng
        lines = []
        for i in range(4):
            self.n[case] += 1
            side = self.n[case] % 2
            s = 1 if (self.n[case] // 2) % 2 else -1
            t = tc + side
            if case == "dp":      # dp = (x + 4) >> 3 = s t
                x = int(r.integers(8 * s * t - 4, 8 * s * t + 4))
            elif case == "dq":    # dq = (4 - x) >> 3 = s t
                x = int(r.integers(-8 * s * t - 3, -8 * s * t + 5))
            elif case == "round":
                x = 8 * s * t - 4 + 8 * side
            elif case == "clip2":   # p0 within tc of one end of the range, q0 near the other
                if tc < 1:
                    return None
                d = int(r.integers(0, tc))
                e = int(r.integers(0, tc))
                p0, q0 = (self.max_v - d, e) if s > 0 else (d, self.max_v - e)
                p1, q1 = int(r.integers(0, self.max_v + 1)), int(r.integers(0, self.max_v + 1))
                lines.append([p0, q0, p1, q1])
                continue
            elif case == "extreme":
                v = [[self.max_v, 0, self.max_v, 0], [0, self.max_v, 0, self.max_v], [self.max_v] * 4, [0] * 4][i]
                lines.append(v)
                continue
            else:
                x = int(r.integers(-16 * (tc + 1), 16 * (tc + 1) + 1))
            ln = self._line_for(x)
            if ln is None:
                return None
            lines.append(ln)
        seg = r.integers(0, self.max_v + 1, (4, 8)).astype(np.int64)
        for i, (p0, q0, p1, q1) in enumerate(lines):
            seg[i, 2], seg[i, 3], seg[i, 4], seg[i, 5] = p1, p0, q0, q1
        return seg


def chroma_plane(bit_depth, rng, *, w=264, h=32, wave="v", qp=30, qp_map=None, ctu_log2=6, tc_table=None):
    """A chroma plane (w x h, multiples of 8) with chroma bS arrays (reference layouts).  wave "v" / "h": as luma_plane, with
    bS 2 on solved segments (bS 1 / 0 sometimes, which chroma skips); wave "default": the default chroma pattern (Q10: what a
    frame's chroma gets), every segment where it has bS 2 solved -- neighbouring segments share samples there, only the
    measured census holds.  The hor2 entry read shifted at bx = w/8 has its Q taps in the picture.
    Returns plane, vert_bs, hor_bs."""
    max_v = (1 << bit_depth) - 1
    plane = rng.integers(max_v // 4, 3 * max_v // 4 + 1, (h, w)).astype(np.int64)
    vs, hs = w // 8 + 1, w // 8
    ops = dict(is_chroma=True, bit_depth=bit_depth, qp=qp, qp_map=qp_map, ctu_log2=ctu_log2, tc_table=tc_table)
    bld = ChromaBuilder(rng, bit_depth)
    k = int(rng.integers(0, 16))

    def solve(seg_kind, bx, by):
        nonlocal k
        ys, xs = segment_coords(seg_kind, bx, by)
        inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
        if not inside[:, 3].any() and not inside[:, 4].any():
            return
        _, tc = (int(v) for v in seg_operands(seg_kind, bx, by, w=w, h=h, **ops))
        seg = None
        for _ in range(len(ChromaBuilder.CASES)):
            seg = bld.build(ChromaBuilder.CASES[k % len(ChromaBuilder.CASES)], tc)
            k += 1
            if seg is not None:
                break
        if seg is None:
            seg = bld.build("small", tc)
        if rng.integers(0, 2):
            seg = seg[:, ::-1]
        _put(plane, seg_kind, bx, by, seg)

    def bs_draw():
        r = int(rng.integers(0, 12))
        return 0 if r == 0 else 1 if r == 1 else 2
    if wave == "default":
        i = np.arange(vs * (h // 8))
        vb = np.where(i % vs == 0, 0, 2).astype(np.uint8).reshape(h // 8, vs)
        i = np.arange((h // 8 + 1) * hs)
        hb = np.where(i % (h // 8 + 1) == 0, 0, 2).astype(np.uint8).reshape(h // 8 + 1, hs)
        for by in range(h // 8 + 1):
            for bx in range(vs):
                for s in range(4):
                    solve(s, bx, by)
    else:
        vb = np.zeros((h // 8, vs), np.uint8)
        hb = np.zeros((h // 8 + 1, hs), np.uint8)
        if wave == "v":
            for r in range(h // 8):
                for bx in range(vs):
                    vb[r, bx] = bs_draw()
                    solve(1, bx, r)
                    solve(0, bx, r + 1)
        else:
            for by in range(h // 8 + 1):
                for c in range(0, hs, 2):
                    hb[by, c] = bs_draw()
                    solve(3, c, by)
                    solve(2, c + 1, by)
            # the shifted read of hor2 at bx = w/8: bS = hor_bs[(by + 1) * hs], Q = the last four columns of row 8 by
            for by in range(h // 8):
                hb[by + 1, 0] = 2
                solve(3, hs, by)
    return plane.astype(np.uint8 if bit_depth == 8 else np.uint16), vb.ravel(), hb.ravel()


# ---- operand sets -----------------------------------------------------------------------------------------------------

def custom_tables():
    """(name, tc table, beta table): beta and tc decoupled -- beta 255 with tc 0, beta 0 with tc at its maximum, odd tc"""
    i = np.arange(52)
    return [("beta255_tc0", np.zeros(52, np.int64), np.full(52, 255, np.int64)),
            ("beta0_tcmax", np.full(52, 255, np.int64), np.zeros(52, np.int64)),
            ("odd_tc", (2 * (i % 13) + 1).astype(np.int64), (i * 5 % 256).astype(np.int64)),
            ("odd_tc_small_beta", (2 * (i % 5) + 1).astype(np.int64), (i % 24).astype(np.int64))]


def packed_tc_fits(max_v, tc_max):
    """deblock_packed.h packed_luma_tc_fits restated from its comment: the strong filter's 5-tap sum with the clip offset,
    8 max_v + 4 + 16 tc, below 2^15 (2^16 for the WIDE 12-bit core); 10 tc and 2 max_v + 1 + 4 tc signed 16-bit"""
    return 8 * max_v + 4 + 16 * tc_max <= (65535 if max_v > 2047 else 32767) and 10 * tc_max <= 32767 and \
        2 * max_v + 1 + 4 * tc_max <= 32767


def fits_edge(bit_depth):
    """the largest table entry (<= 255) whose scaled value the packed luma core holds at this bit depth (-1: none, above 12
    bit the samples alone overflow its fields)"""
    max_v, sh = (1 << bit_depth) - 1, bit_depth - 8
    return max([e for e in range(256) if packed_tc_fits(max_v, e << sh)], default=-1)


def all_qp_map(w, h, ctu_log2, rng, lo=0, hi=51):
    """a QP map whose units take every QP in lo..hi (repeated, shuffled): many distinct (beta, tc) rows in one launch"""
    rows, cols = -(-h >> ctu_log2), -(-w >> ctu_log2)
    v = np.resize(np.arange(lo, hi + 1), rows * cols)
    rng.shuffle(v)
    return v.reshape(rows, cols).astype(np.uint8)


# ---- 8-bit 4:2:0 frames -----------------------------------------------------------------------------------------------

def boundary_frame(w, h, qp, wave, rng):
    """an 8-bit 4:2:0 frame: luma solved for `wave` with its luma bS override, chroma solved under the default chroma
    pattern (the reference's SetBoundaryStrenght leaves chroma bS alone).  Returns y, u, v, vert_bs, hor_bs."""
    y, vb, hb = luma_plane(8, rng, w=w, h=h, wave=wave, qp=qp)
    u, _, _ = chroma_plane(8, rng, w=w // 2, h=h // 2, wave="default", qp=qp)
    v, _, _ = chroma_plane(8, rng, w=w // 2, h=h // 2, wave="default", qp=qp)
    return y, u, v, vb, hb
