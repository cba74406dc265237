"""slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation: the decision under a flag pair per slice, the totals per slice and
pair, the choice and the final decision -- the rule of include/hevc_deblock.h in Python ints, on top of sao_scale_ref.Decider.

TEST INFRASTRUCTURE ONLY, parity unpinned like the rest of SAO.  Written from the header's text; nothing of the library is mentioned
here.  A pair is c = L + 2 C.  A CTB under pair 0 has no candidate, "not applied" in every component and an all-zero record; under
another pair its NEW candidate loses the part whose flag is 0 -- "not applied" at a cost of 0 -- and the serial walk of
sao_decide_ref.Decider goes on as it is.  Totals are Python ints: nothing wraps.
"""
import numpy as np

import rext_oracle as ro
import sao_decide_ref as D
import sao_scale_ref as R


class Decider(R.Decider):
    """sao_scale_ref.Decider whose decide() takes the flags: an int (every slice the same pair) or a sequence indexed by slice"""

    def new_under(self, k, pair):
        (py, pcb, pcr), c_y, c_c, _ = self.new(k)
        L, C = pair & 1, (pair >> 1) & 1 if self.chroma else 0
        return (py if L else D.OFF, pcb if C else D.OFF, pcr if C else D.OFF), c_y if L else 0, c_c if C else 0

    def pair_of(self, flags, s, n_slices):
        """the pair of a CTB of slice s: 0 beyond n_slices, bit 1 counts with chroma alone, higher bits do not count"""
        if n_slices is not None and s >= n_slices:
            return 0
        return (flags if isinstance(flags, int) else int(flags[s])) & (3 if self.chroma else 1)

    def decide(self, idx, slice_idx=None, tile_idx=None, flags=3, n_slices=None):
        """as sao_decide_ref.Decider.decide, every CTB under the pair of its slice (slice_idx None: slice 0)"""
        rows, cols = idx.shape
        final = [[None] * cols for _ in range(rows)]
        dec = np.zeros((rows, cols), D.DECISION_DTYPE)
        j_of = np.zeros((rows, cols), object)
        for cy in range(rows):
            for cx in range(cols):
                k = int(idx[cy, cx])
                pair = self.pair_of(flags, 0 if slice_idx is None else int(slice_idx[cy, cx]), n_slices)
                if pair == 0:
                    final[cy][cx] = (D.OFF, D.OFF, D.OFF)      # the record stays all zero, J = 0
                    j_of[cy, cx] = 0
                    continue
                cand = D.candidates(cx, cy, slice_idx, tile_idx)
                triple, c_y, c_c = self.new_under(k, pair)
                F = (cand & 1) + (cand >> 1)
                best = (self.J(c_y, c_c, F), 0, triple, c_y, c_c, F)
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
                dd = D.pd(sy, t[0]) + (D.pd(scb, t[1]) + D.pd(scr, t[2]) if self.chroma else 0)
                dec[cy, cx] = (dd, c_y, c_c, m, F, cand, (0,) * 5)
        params = []
        for c in range(3 if self.chroma else 1):
            p = np.zeros((rows, cols), ro.SAO_CTB_DTYPE)
            for cy in range(rows):
                for cx in range(cols):
                    p[cy, cx] = final[cy][cx][c]
            params.append(p)
        return {"params": params + [None] * (3 - len(params)), "decision": dec, "j": j_of}

    def totals(self, idx, slice_idx, tile_idx, n_slices):
        """T[s][c]: the sum of the chosen J over the CTBs of slice s with every slice under pair c; and the CTBs per slice"""
        T = [[0, 0, 0, 0] for _ in range(n_slices)]
        count = [0] * n_slices
        sl = np.zeros(idx.shape, np.int64) if slice_idx is None else slice_idx
        for c in (1, 2, 3) if self.chroma else (1,):
            j = self.decide(idx, slice_idx, tile_idx, c, n_slices)["j"]
            for cy in range(idx.shape[0]):
                for cx in range(idx.shape[1]):
                    if sl[cy, cx] < n_slices:
                        T[int(sl[cy, cx])][c] += int(j[cy, cx])
                        count[int(sl[cy, cx])] += c == 1
        return T, count

    def choose(self, idx, slice_idx, tile_idx, n_slices, *, wrap=None):
        """{"flags": the pair per slice -- the least T in the order 0, 1, 2, 3, the earliest on a tie; "T", "n_ctbs"; and the final
        decision's "params", "decision", "j"}.  wrap: compare the totals wrapped to that many bits (what the rule does NOT do)"""
        T, count = self.totals(idx, slice_idx, tile_idx, n_slices)

        def seen(t):
            if wrap is None:
                return t
            t &= (1 << wrap) - 1
            return t - (1 << wrap) if t >> (wrap - 1) else t
        flags = [min(range(4 if self.chroma else 2), key=lambda c: (seen(T[s][c]), c)) for s in range(n_slices)]
        out = self.decide(idx, slice_idx, tile_idx, flags, n_slices)
        out.update(flags=flags, T=T, n_ctbs=count)
        return out


SLICE_RECORD_DTYPE = np.dtype([("cost_lo", "<u8", (4,)), ("cost_hi", "<i8", (4,)), ("n_ctbs", "<u4"), ("flags", "u1"), ("zero", "u1", (3,))])
assert SLICE_RECORD_DTYPE.itemsize == 72


def records(res):
    """the slice records of a choose() result: T as 128-bit two's complement numbers"""
    out = np.zeros(len(res["flags"]), SLICE_RECORD_DTYPE)
    for s, (T, n, fl) in enumerate(zip(res["T"], res["n_ctbs"], res["flags"])):
        for c in range(4):
            u = T[c] & ((1 << 128) - 1)
            out[s]["cost_lo"][c] = u & ((1 << 64) - 1)
            hi = u >> 64
            out[s]["cost_hi"][c] = hi - (1 << 64) if hi >> 63 else hi
        out[s]["n_ctbs"], out[s]["flags"] = n, fl
    return out
