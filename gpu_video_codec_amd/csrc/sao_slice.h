/*
 * sao_slice.h -- slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation (hevcdbk_sao_decide_device_sf,
 * hevcdbk_sao_slice_flags_device; the kernels around it are sao_slice.hip): the decision of sao_pick_os.h / sao_decide.h under a flag
 * pair per slice, and the choice of that pair.  The rule is in include/hevc_deblock.h, in plain ints in tests/sao_slice_ref.py.
 *
 * A flag pair c = L + 2 C masks the NEW candidate of a CTB: without L the luma part is "not applied" at a cost of 0, without C the
 * chroma part; with neither the CTB has no candidate and an all-zero record (new_masked).  LEFT, UP and the walk are sao_decide.h's,
 * unchanged: a merge candidate lies in the CTB's own slice, so it was masked by the same pair.
 *
 * The choice: the workspace holds one complete state of the decision -- three parameter grids and the records -- per pair 1, 2, 3
 * (without chroma: pair 1 alone).  NEW writes the two picks of a CTB, computed once, into the three states under the three masks;
 * the walk runs merge_ctb on each state (pair_state) and adds the chosen candidate's J, as four 32-bit limbs, into 64-bit sums per
 * slice, pair and limb (limb, sum_at): at most 2^32 CTBs of less than 2^32 each, so no sum wraps, and integer sums are the same in any
 * order.  choose() propagates the carries into a 128-bit total per pair and takes the least, the earliest on a tie; final_ctb copies a
 * CTB's entries from the state of its slice's pair.  The kernels and tests/sao_slice_sim run these functions in the same order (DBK_HD).
 */
#pragma once
#include <stdint.h>

#include "sao_pick_os.h"

/* hevcdbk_sao_slice_record of the C ABI */
struct DbkSaoSliceRecord {
    uint64_t cost_lo[4];
    int64_t cost_hi[4];
    uint32_t n_ctbs;
    uint8_t flags, zero[3];
};

/* the operands of the launches of sao_slice.hip: those of the _os decision (o.d's outputs are the caller's), then the flags */
struct DbkSaoSliceArgs {
    DbkSaoDecideOsArgs o;
    int n_slices;
    long long flags_frame_stride; /* bytes; 0 = shared (an input only) */
    const uint8_t *flags_in;      /* the decision under given flags */
    uint8_t *flags_out;           /* the choice: [frame][slice] */
    DbkSaoSliceRecord *record;    /* may be NULL */
    long long record_frame_stride;
    DbkSaoDecision *ws_decision; /* the workspace: [frame][pair - 1][ctb] */
    DbkSaoCtb *ws_params;        /* [frame][pair - 1][component][ctb] */
};

namespace saoslice {

using saodecide::wide;

constexpr int kMaxSlices = 600;  /* of the choosing entry: MaxSliceSegmentsPerPicture at the highest levels */
constexpr int kSums = 12;        /* 64-bit sums per slice: pairs 1..3 x four limbs */
constexpr int kStateBytes = 3 * (int)(sizeof(DbkSaoDecision) + 3 * sizeof(DbkSaoCtb)); /* of the workspace per CTB and frame */

DBK_HD int pairs(const DbkSaoSliceArgs &s) { return s.o.d.stats_cb ? 3 : 1; }

DBK_HD unsigned slice_of(const DbkSaoDecideArgs &a, int f, int cx, int cy)
{
    return a.slice_idx ? a.slice_idx[(long long)f * a.idx_frame_stride + (long long)cy * a.idx_stride + cx] : 0u;
}

/* the pair a CTB decides under, from the caller's flag bytes: 0 beyond n_slices; bit 1 counts with chroma statistics alone */
DBK_HD unsigned pair_given(const DbkSaoSliceArgs &s, int f, int cx, int cy)
{
    const unsigned sl = slice_of(s.o.d, f, cx, cy);
    if (sl >= (unsigned)s.n_slices) return 0u;
    return s.flags_in[(long long)f * s.flags_frame_stride + sl] & (s.o.d.stats_cb ? 3u : 1u);
}

/* lane 0 of a NEW wave: saoos::write_new under the pair -- the triple and the whole record into a's outputs */
DBK_HD void new_masked(const DbkSaoDecideArgs &a, int f, int cx, int cy, const saoos::BinPick *py, const saoos::BinPick *pcb, const saoos::BinPick *pcr,
                       const saoos::Choice &y, const saoos::Choice &c, unsigned pair)
{
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    DbkSaoDecision r = {};
    DbkSaoCtb ctb = {};
    if (pair & 1u) {
        r.delta_d = saoos::write_ctb(py, y.type, y.cls_a, ctb);
        r.cost_luma = y.cost;
    }
    a.params_y[out] = ctb;
    if (a.stats_cb) {
        DbkSaoCtb cb = {}, cr = {};
        if (pair & 2u) {
            r.delta_d += saoos::write_ctb(pcb, c.type, c.cls_a, cb);
            r.delta_d += saoos::write_ctb(pcr, c.type, c.cls_b, cr);
            r.cost_chroma = c.cost;
        }
        a.params_cb[out] = cb;
        a.params_cr[out] = cr;
    }
    if (pair) {
        r.cand = (uint8_t)saodecide::candidates(a, f, cx, cy);
        r.flag_bits = (uint8_t)saodecide::flag_count(r.cand);
    }
    a.decision[(long long)f * a.decision_frame_stride + (long long)cy * a.decision_stride + cx] = r;
}

/* the operands of the decision with the state of `pair` (1..3) in the workspace as its outputs: tight grids */
DBK_HD DbkSaoDecideArgs pair_state(const DbkSaoSliceArgs &s, int pair)
{
    DbkSaoDecideArgs w = s.o.d;
    const long long n = (long long)w.ctbs_x * w.ctbs_y;
    w.params_stride = w.decision_stride = w.ctbs_x;
    w.decision_frame_stride = 3 * n;
    w.params_frame_stride = 9 * n;
    w.decision = s.ws_decision + (pair - 1) * n;
    w.params_y = s.ws_params + (pair - 1) * 3 * n;
    w.params_cb = w.params_y + n;
    w.params_cr = w.params_cb + n;
    return w;
}

/* lane 0 of the choosing entry's NEW wave: the picks into every state, each under its pair; a CTB beyond n_slices has none */
DBK_HD void new_states(const DbkSaoSliceArgs &s, int f, int cx, int cy, const saoos::BinPick *py, const saoos::BinPick *pcb, const saoos::BinPick *pcr,
                       const saoos::Choice &y, const saoos::Choice &c)
{
    const bool in = slice_of(s.o.d, f, cx, cy) < (unsigned)s.n_slices;
    for (int pair = 1; pair <= pairs(s); pair++) new_masked(pair_state(s, pair), f, cx, cy, py, pcb, pcr, y, c, in ? (unsigned)pair : 0u);
}

/* one CTB of the walk in the state w = pair_state(): merge_ctb, then J of the candidate it ended up with */
DBK_HD wide walk_ctb(const DbkSaoDecideArgs &w, int f, int cx, int cy)
{
    saodecide::merge_ctb(w, f, cx, cy);
    const DbkSaoDecision &r = w.decision[(long long)f * w.decision_frame_stride + (long long)cy * w.decision_stride + cx];
    return saodecide::rd_cost(w, r.cost_luma, r.cost_chroma, r.flag_bits);
}

/* limb i of J as a 128-bit two's complement number; where it is added */
DBK_HD uint32_t limb(wide j, int i) { return (uint32_t)((unsigned __int128)j >> (32 * i)); }
DBK_HD int sum_at(unsigned slice, int pair, int i) { return ((int)slice * 3 + (pair - 1)) * 4 + i; }

/* one slice of one frame, from its twelve sums: the totals with the carries propagated, the least of T_0 = 0, T_1, T_2, T_3 in
 * this order (without chroma T_0, T_1), the earliest on a tie.  Fills the record; returns the flags */
DBK_HD unsigned choose(const unsigned long long *sums, unsigned n_ctbs, bool chroma, DbkSaoSliceRecord &rec)
{
    rec = DbkSaoSliceRecord{};
    unsigned best = 0;
    wide least = 0;
    for (int pair = 1; pair <= (chroma ? 3 : 1); pair++) {
        unsigned long long carry = 0, out[4];
        for (int i = 0; i < 4; i++) {
            const unsigned long long t = sums[(pair - 1) * 4 + i] + carry; /* below 2^64: a sum is at most 2^32 * (2^32 - 1) */
            out[i] = t & 0xffffffffull;
            carry = t >> 32;
        }
        rec.cost_lo[pair] = out[0] | (out[1] << 32);
        rec.cost_hi[pair] = (int64_t)(out[2] | (out[3] << 32));
        const wide total = (wide)(((unsigned __int128)(uint64_t)rec.cost_hi[pair] << 64) | rec.cost_lo[pair]);
        if (total < least) {
            least = total;
            best = (unsigned)pair;
        }
    }
    rec.n_ctbs = n_ctbs;
    rec.flags = (uint8_t)best;
    return best;
}

/* the final entries of one CTB: those of the state of its slice's pair, or "not applied" and an all-zero record */
DBK_HD void final_ctb(const DbkSaoSliceArgs &s, int f, int cx, int cy)
{
    const DbkSaoDecideArgs &a = s.o.d;
    const unsigned sl = slice_of(a, f, cx, cy);
    const unsigned pair = sl < (unsigned)s.n_slices ? s.flags_out[(long long)f * s.flags_frame_stride + sl] : 0u;
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    DbkSaoCtb y = {}, cb = {}, cr = {};
    DbkSaoDecision r = {};
    if (pair) {
        const DbkSaoDecideArgs w = pair_state(s, (int)pair);
        const long long at = (long long)f * w.params_frame_stride + (long long)cy * w.params_stride + cx;
        y = w.params_y[at];
        if (a.stats_cb) {
            cb = w.params_cb[at];
            cr = w.params_cr[at];
        }
        r = w.decision[(long long)f * w.decision_frame_stride + (long long)cy * w.decision_stride + cx];
    }
    a.params_y[out] = y;
    if (a.stats_cb) {
        a.params_cb[out] = cb;
        a.params_cr[out] = cr;
    }
    a.decision[(long long)f * a.decision_frame_stride + (long long)cy * a.decision_stride + cx] = r;
}

} /* namespace saoslice */
