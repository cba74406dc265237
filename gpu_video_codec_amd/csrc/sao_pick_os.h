/*
 * sao_pick_os.h -- SAO parameter estimation with log2_sao_offset_scale (hevcdbk_sao_pick_device_os, hevcdbk_sao_decide_device_os; the
 * kernels around it are sao_pick_os.hip): the pick rule of sao_stats.h with offsets coded in units of 2^k, and the choice of a CTB's
 * candidate shared by the lanes of a wave.  The rule is in include/hevc_deblock.h, in plain ints in tests/sao_scale_ref.py.
 *
 * What a wave does for one CTB, written as what ONE LANE does in each step (DBK_HD, as sao_stats.h); between the steps the lanes
 * exchange keys -- cross-lane moves in the kernel, an array of 64 keys in tests/sao_scale_sim, which runs every step for all 64 lanes:
 *   1. lanes 0..47: pick_bin -- the offset of one bin, in coded units q, stored scaled (o = q * 2^k) with its cost and distortion;
 *   2. every lane: the key of ITS candidate -- single_key (lane 0 "not applied", 1..4 the edge classes, 5..36 the band positions) or,
 *      for Cr beside Cb, joint_edge_key (lane 0 "not applied", 1..4 the edge classes) and joint_band_key (lanes 0..31 Cb's band
 *      positions, 32..63 Cr's);
 *   3. the exchange: key_min with the key of lane ^ 1, ^ 2, ... -- after it every lane of a group holds the group's least key;
 *   4. every lane: single_choice / joint_choice -- the candidate the least key names; lane 0: write_ctb -- the four offsets and the
 *      distortion from the winning candidate's bins.
 * A key is cost * 64 + index in one int64: the least key is the lowest cost and, on a tie, the lowest index -- "the earliest".  A bin's
 * cost is below 2^54 (n < 2^31, |o| <= 124, lambda <= 2^24), so four bins and lambda * 7 stay below 2^57, times 64 below 2^63; the
 * joint edge candidates -- eight bins and lambda * 4, below 2^58 -- are five, and their key is cost * 8 + index (joint_edge_key).
 */
#pragma once
#include <stdint.h>

#include "sao_decide.h"
#include "sao_stats.h"

/* the operands of the launches of sao_pick_os.hip: those of the kernels without a scale, unchanged, and the scales beside them */
struct DbkSaoPickOsArgs {
    DbkSaoPickArgs p;
    int log2_scale; /* k: 0..2 */
};
struct DbkSaoDecideOsArgs {
    DbkSaoDecideArgs d;
    int log2_scale_luma, log2_scale_chroma; /* 0..2 each */
};

namespace saoos {

using saostats::BinPick;

/* the coded offset q of a bin (n samples, sum s of org - rec) at scale k: the mean divided by 2^k, rounded half away from zero in ONE
 * division, clamped to [lo, hi], then walked towards 0; the least (n o^2 - 2 o s) * 256 + lambda * bits(q) with o = q * 2^k wins, on a
 * tie the q nearer 0.  Returns q; cost out.  k = 0 is saostats::pick_offset */
DBK_HD int pick_offset(long long n, long long s, int k, int lo, int hi, int M, bool band, long long lambda, long long &cost)
{
    if (n == 0) {
        cost = lambda * saostats::offset_bits(0, M, band);
        return 0;
    }
    const long long as = s < 0 ? -s : s, nk = n * (1ll << k), unit = 1ll << k;
    long long q0 = (2 * as + nk) / (2 * nk);
    if (s < 0) q0 = -q0;
    if (q0 < lo) q0 = lo;
    if (q0 > hi) q0 = hi;
    int best = (int)q0;
    long long best_cost = 0;
    for (long long q = q0;; q += q > 0 ? -1 : 1) {
        const long long o = q * unit;
        const long long c = (n * o * o - 2 * o * s) * 256 + lambda * saostats::offset_bits((int)q, M, band);
        if (q == q0 || c <= best_cost) {
            best = (int)q;
            best_cost = c;
        }
        if (q == 0) break;
    }
    cost = best_cost;
    return best;
}

/* bin 0..47 of a CTB (saostats::pick_bin's order and limits) at scale k: o is SaoOffsetVal = q * 2^k, dd and cost are taken on it */
DBK_HD BinPick pick_bin(const int32_t *st, int bin, int M, int k, long long lambda)
{
    const bool band = bin >= 16;
    const long long n = band ? st[saostats::kBoCount + bin - 16] : st[saostats::kEoCount + bin];
    const long long s = band ? st[saostats::kBoSum + bin - 16] : st[saostats::kEoSum + bin];
    const int lo = band ? -M : ((bin & 3) < 2 ? 0 : -M), hi = band ? M : ((bin & 3) < 2 ? M : 0);
    BinPick p;
    p.o = pick_offset(n, s, k, lo, hi, M, band, lambda, p.cost) * (1 << k);
    p.dd = saostats::delta_d(n, s, p.o);
    return p;
}

/* ---- keys ---------------------------------------------------------------------------------------------------------------------- */

typedef long long Key;
constexpr Key kNoKey = INT64_MAX; /* a lane without a candidate: above every key there is */

DBK_HD Key make_key(long long cost, int idx) { return cost * 64 + idx; } /* a multiplication: the cost may be negative */
DBK_HD int key_idx(Key k) { return (int)(k & 63); }
DBK_HD long long key_cost(Key k) { return (k - (k & 63)) / 64; } /* exact */
DBK_HD Key key_min(Key a, Key b) { return b < a ? b : a; }

DBK_HD long long edge_cost(const BinPick *p, int c) { return p[4 * c].cost + p[4 * c + 1].cost + p[4 * c + 2].cost + p[4 * c + 3].cost; }
DBK_HD long long band_cost(const BinPick *p, int pos)
{
    return p[16 + (pos & 31)].cost + p[16 + ((pos + 1) & 31)].cost + p[16 + ((pos + 2) & 31)].cost + p[16 + ((pos + 3) & 31)].cost;
}

/* one component: the candidate of a lane, index = lane -- the order of the rule */
DBK_HD Key single_key(const BinPick *p, int lane, long long lambda)
{
    if (lane == 0) return make_key(lambda, 0);
    if (lane < 5) return make_key(lambda * 4 + edge_cost(p, lane - 1), lane);
    if (lane < 37) return make_key(lambda * 7 + band_cost(p, lane - 5), lane);
    return kNoKey;
}

/* Cr (b) beside Cb (a): "not applied" and the four edge classes over both components.  Eight bins reach 2^57, so the key is formed
 * as cost * 8 + index -- three bits hold the five candidates -- and read back by joint_edge_* below */
DBK_HD Key joint_edge_key(const BinPick *a, const BinPick *b, int lane, long long lambda)
{
    if (lane == 0) return lambda * 8;
    if (lane < 5) return (lambda * 4 + edge_cost(a, lane - 1) + edge_cost(b, lane - 1)) * 8 + lane;
    return kNoKey;
}
DBK_HD int joint_edge_idx(Key k) { return (int)(k & 7); }
DBK_HD long long joint_edge_cost(Key k) { return (k - (k & 7)) / 8; }

/* lanes 0..31: Cb's band position `lane`; lanes 32..63: Cr's band position lane - 32.  The least key of each half: that component's
 * best position, on a tie the lowest */
DBK_HD Key joint_band_key(const BinPick *a, const BinPick *b, int lane) { return make_key(band_cost(lane < 32 ? a : b, lane & 31), lane & 31); }

/* ---- from the least keys to the parameters --------------------------------------------------------------------------------------- */

struct Choice {
    int type, cls_a, cls_b; /* cls_b: Cr's band position in the joint form; else cls_a */
    long long cost;
};

DBK_HD Choice single_choice(Key least)
{
    const int i = key_idx(least);
    Choice c;
    c.type = i == 0 ? 0 : (i < 5 ? 2 : 1);
    c.cls_a = c.cls_b = i == 0 ? 0 : (i < 5 ? i - 1 : i - 5);
    c.cost = key_cost(least);
    return c;
}

/* edge: the least joint_edge_key; band_a, band_b: the least joint_band_key of each half.  The band form costs lambda * 2 plus per
 * component lambda * 5 and wins only when strictly less than everything before it */
DBK_HD Choice joint_choice(Key edge, Key band_a, Key band_b, long long lambda)
{
    const long long band = lambda * 12 + key_cost(band_a) + key_cost(band_b), before = joint_edge_cost(edge);
    const int i = joint_edge_idx(edge);
    Choice c;
    if (band < before) {
        c.type = 1; c.cls_a = key_idx(band_a); c.cls_b = key_idx(band_b); c.cost = band;
    } else {
        c.type = i == 0 ? 0 : 2; c.cls_a = c.cls_b = i == 0 ? 0 : i - 1; c.cost = before;
    }
    return c;
}

/* the parameters of one component from the bins of the chosen candidate; returns the distortion they predict */
DBK_HD long long write_ctb(const BinPick *p, int type, int cls, DbkSaoCtb &out)
{
    long long dd = 0;
    out.type = (uint8_t)type;
    out.cls = (uint8_t)cls;
    for (int k = 0; k < 4; k++) {
        const BinPick *q = type == 2 ? &p[4 * cls + k] : (type == 1 ? &p[16 + ((cls + k) & 31)] : nullptr);
        out.offset[k] = (int8_t)(q ? q->o : 0);
        dd += q ? q->dd : 0;
    }
    return dd;
}

/* lane 0 of the pick wave: the parameters and delta_d of a CTB.  b == nullptr: one component, c from single_choice */
DBK_HD void write_pick(const DbkSaoPickArgs &a, int f, int cx, int cy, const BinPick *pa, const BinPick *pb, const Choice &c)
{
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    DbkSaoCtb ctb;
    long long dd = write_ctb(pa, c.type, c.cls_a, ctb);
    a.params_a[out] = ctb;
    if (pb) {
        dd += write_ctb(pb, c.type, c.cls_b, ctb);
        a.params_b[out] = ctb;
    }
    if (a.delta_d) a.delta_d[((long long)f * a.ctbs_y + cy) * a.ctbs_x + cx] = dd;
}

/* lane 0 of the decision's NEW wave: the triple and the whole record, as saodecide::new_ctb writes them.  y from single_choice on
 * luma's bins, c from joint_choice on Cb's and Cr's (not looked at without chroma) */
DBK_HD void write_new(const DbkSaoDecideArgs &a, int f, int cx, int cy, const BinPick *py, const BinPick *pcb, const BinPick *pcr, const Choice &y,
                      const Choice &c)
{
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    DbkSaoDecision r = {};
    DbkSaoCtb ctb;
    r.delta_d = write_ctb(py, y.type, y.cls_a, ctb);
    r.cost_luma = y.cost;
    a.params_y[out] = ctb;
    if (a.stats_cb) {
        r.delta_d += write_ctb(pcb, c.type, c.cls_a, ctb);
        a.params_cb[out] = ctb;
        r.delta_d += write_ctb(pcr, c.type, c.cls_b, ctb);
        a.params_cr[out] = ctb;
        r.cost_chroma = c.cost;
    }
    r.cand = (uint8_t)saodecide::candidates(a, f, cx, cy);
    r.flag_bits = (uint8_t)saodecide::flag_count(r.cand);
    a.decision[(long long)f * a.decision_frame_stride + (long long)cy * a.decision_stride + cx] = r;
}

} /* namespace saoos */
