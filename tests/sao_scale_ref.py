"""SAO estimation with log2_sao_offset_scale (hevcdbk_sao_pick_device_os, hevcdbk_sao_decide_device_os): the rule of
include/hevc_deblock.h with a scale k, pick and decision, in Python ints.

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of SAO.  Written from the header's text; nothing of the library is mentioned
here.  A bin's offset is chosen in coded units q and stored as o = q * 2^k; every cost and every distortion is taken on o.  The
candidates of a CTB are listed with their costs and the minimum is taken over (cost, position in the list): the lowest cost, on a tie
the earliest.  The decision is sao_decide_ref.Decider's serial walk with this pick as NEW: LEFT and UP work on the stored offsets.
"""
import numpy as np

import rext_oracle as ro
import sao_decide_ref as D
import sao_stats_ref as S


def max_offset(bit_depth):
    return (1 << (min(bit_depth, 10) - 5)) - 1


def max_scale(bit_depth):
    """the largest log2_sao_offset_scale a stream codes at this depth"""
    return max(0, bit_depth - 10)


def bits(q, M, band):
    return (abs(q) + 1 if abs(q) < M else M) + (1 if band and q != 0 else 0)


def sign(v):
    return (v > 0) - (v < 0)


def offset_trace(n, s, k, lo, hi, M, band, lam):
    """the offset of a bin, with the steps on the way: {"q0": the rounded scaled mean, "start": q0 clamped, "q": the q kept, "o", "cost",
    "dd"}"""
    if n == 0:
        return {"q0": 0, "start": 0, "q": 0, "o": 0, "cost": lam * bits(0, M, band), "dd": 0}
    nk = n << k
    q0 = sign(s) * ((2 * abs(s) + nk) // (2 * nk))
    start = min(max(q0, lo), hi)
    best = None
    q = start
    while True:
        o = q * 2 ** k
        dd = n * o * o - 2 * o * s
        cost = dd * 256 + lam * bits(q, M, band)
        if best is None or cost <= best[1]:           # walking towards 0: an equal cost later is the q nearer 0
            best = (q, cost, dd)
        if q == 0:
            break
        q -= sign(q)
    return {"q0": q0, "start": start, "q": best[0], "o": best[0] * 2 ** k, "cost": best[1], "dd": best[2]}


def bin_limits(e, M):
    """edge category e + 1: 1 and 2 take 0..M, 3 and 4 take -M..0"""
    return (0, M) if e < 2 else (-M, 0)


def bins(st, M, k, lam):
    """per component: edge[c][e] and band[b], each an offset_trace"""
    edge = [[offset_trace(int(st["eo_count"][c][e]), int(st["eo_sum"][c][e]), k, *bin_limits(e, M), M, False, lam) for e in range(4)] for c in range(4)]
    band = [offset_trace(int(st["bo_count"][b]), int(st["bo_sum"][b]), k, -M, M, M, True, lam) for b in range(32)]
    return edge, band


def pick_ctb(st_a, st_b, bit_depth, lam, k):
    """the choice of one CTB (st_b: Cr beside Cb, or None): ([(type, cls, offsets) per component], delta_d, the least cost)"""
    M = max_offset(bit_depth)
    comps = [bins(s, M, k, lam) for s in ((st_a,) if st_b is None else (st_a, st_b))]
    four = lambda c, p: [c[1][(p + j) & 31] for j in range(4)]
    cost_of = lambda chosen: sum(b["cost"] for b in chosen)
    cands = [(lam * 1, 0, None)]
    for c in range(4):
        cands.append((lam * 4 + sum(cost_of(comp[0][c]) for comp in comps), 2, (c,) * len(comps)))
    if st_b is None:
        for p in range(32):
            cands.append((lam * 7 + cost_of(four(comps[0], p)), 1, (p,)))
    else:
        pos, cost = [], lam * 2
        for comp in comps:
            least = min((cost_of(four(comp, p)), p) for p in range(32))     # the lowest position on a tie
            pos.append(least[1])
            cost += lam * 5 + least[0]
        cands.append((cost, 1, tuple(pos)))                                   # last: it wins only when strictly less
    cost, typ, arg = min(cands, key=lambda c: c[0])                          # min() keeps the first of equals
    out, dd = [], 0
    for i, comp in enumerate(comps):
        if typ == 0:
            out.append((0, 0, (0, 0, 0, 0)))
            continue
        chosen = comp[0][arg[i]] if typ == 2 else four(comp, arg[i])
        out.append((typ, arg[i], tuple(b["o"] for b in chosen)))
        dd += sum(b["dd"] for b in chosen)
    return out, dd, cost


def pick_plane(stats_a, stats_b, bit_depth, lam, k):
    """pick_ctb over a grid: (params_a, params_b or None, delta_d)"""
    rows, cols = stats_a.shape
    pa, pb = np.zeros((rows, cols), ro.SAO_CTB_DTYPE), None if stats_b is None else np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
    dd = np.zeros((rows, cols), np.int64)
    memo = {}
    for r in range(rows):
        for c in range(cols):
            key = stats_a[r, c].tobytes() + (b"" if stats_b is None else stats_b[r, c].tobytes())
            if key not in memo:
                memo[key] = pick_ctb(stats_a[r, c], None if stats_b is None else stats_b[r, c], bit_depth, lam, k)
            out, dd[r, c], _ = memo[key]
            for p, o in zip((pa, pb), out):
                p[r, c] = o
    return pa, pb, dd


class Decider(D.Decider):
    """sao_decide_ref.Decider with the scaled pick as NEW; the walk, J, the candidates and the merge costs are inherited"""

    def __init__(self, palette, *, k_luma=0, k_chroma=None, **kw):
        D.Decider.__init__(self, palette, **kw)
        self.k_l, self.k_c = k_luma, k_luma if k_chroma is None else k_chroma

    def new(self, k):
        if k not in self._new:
            sy, scb, scr = self.palette[k]
            (py,), dy, cy = pick_ctb(sy, None, self.bd_l, self.lam_l, self.k_l)
            if self.chroma:
                (pcb, pcr), dc, cc = pick_ctb(scb, scr, self.bd_c, self.lam_c, self.k_c)
            else:
                pcb, pcr, dc, cc = D.OFF, D.OFF, 0, 0
            self._new[k] = ((py, pcb, pcr), cy, cc, dy + dc)
        return self._new[k]
