/*
 * sao_decide.h -- the SAO decision per CTB (hevcdbk_sao_decide_device; the kernels around it are sao_decide.hip): own parameters,
 * sao_merge_left_flag or sao_merge_up_flag (H.265 7.3.8.3) over Y, Cb and Cr at once.  The rule is in include/hevc_deblock.h, in plain
 * ints in tests/sao_decide_ref.py.
 *
 * Two steps.  new_ctb: what one CTB does on its own -- the NEW triple from the pick rule (sao_stats.h) into params_*, its costs and
 * the candidates that exist into the record.  merge_ctb: what one CTB does once its left and upper neighbours are FINAL -- weighs
 * their triples against its own and, where one wins, copies that triple and rewrites the record.  A CTB depends on the two
 * neighbours of the anti-diagonal before its own (cx + cy - 1) and on nothing else, so the CTBs of one anti-diagonal are
 * independent: diagonal() names them.  The kernel and tests/sao_decide_sim walk the diagonals in the same order with the same
 * functions (DBK_HD, as sao_stats.h).
 *
 * The compared quantity J = lambda_c * C_y + lambda_l * C_c + lambda_l * lambda_c * F passes 64 bits (costs reach 2^48 with sums at
 * the int32 extremes, lambdas 2^24): it is formed and compared in __int128 -- multiplications, additions, one comparison.
 */
#pragma once
#include <stdint.h>

#include "sao_stats.h"

/* hevcdbk_sao_decision of the C ABI */
struct DbkSaoDecision {
    long long delta_d, cost_luma, cost_chroma;
    uint8_t merge, flag_bits, cand, zero[5];
};

/* the operands of the two launches (sao_decide.hip) as the host entry fills them (sao_decide_host.cpp).  Plain data */
struct DbkSaoDecideArgs {
    const int32_t *stats_y, *stats_cb, *stats_cr; /* 96 int32 per CTB; stats_cb == NULL: luma alone */
    int stats_stride;
    long long stats_frame_stride; /* entries; 0 = shared */
    int ctbs_x, ctbs_y, n_frames;
    int max_offset_luma, max_offset_chroma; /* M = (1 << (Min(bitDepth, 10) - 5)) - 1 */
    long long lambda_luma, lambda_chroma;
    const uint16_t *slice_idx, *tile_idx; /* either may be NULL */
    int idx_stride;
    long long idx_frame_stride;
    DbkSaoCtb *params_y, *params_cb, *params_cr;
    int params_stride;
    long long params_frame_stride;
    DbkSaoDecision *decision;
    int decision_stride;
    long long decision_frame_stride;
};

namespace saodecide {

typedef __int128 wide;

constexpr unsigned kLeft = 1u, kUp = 2u; /* bits of `cand`, and the values of `merge` */
constexpr int kChunk = 256;              /* CTBs of a diagonal taken at a time: the threads of the merge kernel's workgroup */

/* bit 0: a left candidate exists -- cx > 0 and the left CTB has this CTB's slice index and tile index; bit 1: likewise the upper */
DBK_HD unsigned candidates(const DbkSaoDecideArgs &a, int f, int cx, int cy)
{
    const long long at = (long long)f * a.idx_frame_stride + (long long)cy * a.idx_stride + cx;
    auto same = [&](long long nb) { return (!a.slice_idx || a.slice_idx[at] == a.slice_idx[nb]) && (!a.tile_idx || a.tile_idx[at] == a.tile_idx[nb]); };
    return (cx > 0 && same(at - 1) ? kLeft : 0u) | (cy > 0 && same(at - a.idx_stride) ? kUp : 0u);
}

/* pd(S, p): the sum over the four bins p uses of n o^2 - 2 o s */
DBK_HD long long predicted(const int32_t *st, const DbkSaoCtb &p)
{
    long long d = 0;
    if (p.type != 1 && p.type != 2) return 0;
    for (int k = 0; k < 4; k++) {
        const int e = 4 * (p.cls & 3) + k, b = (p.cls + k) & 31;
        const long long n = p.type == 2 ? st[saostats::kEoCount + e] : st[saostats::kBoCount + b];
        const long long s = p.type == 2 ? st[saostats::kEoSum + e] : st[saostats::kBoSum + b];
        d += saostats::delta_d(n, s, p.offset[k]);
    }
    return d;
}

/* J of a candidate with costs C_y, C_c and F flag bits; without chroma C_y + lambda_l * F */
DBK_HD wide rd_cost(const DbkSaoDecideArgs &a, long long c_y, long long c_c, int flag_bits)
{
    if (!a.stats_cb) return (wide)c_y + (wide)a.lambda_luma * flag_bits;
    return (wide)a.lambda_chroma * c_y + (wide)a.lambda_luma * c_c + (wide)a.lambda_luma * a.lambda_chroma * flag_bits;
}

DBK_HD int flag_count(unsigned cand) { return (int)(cand & 1u) + (int)((cand >> 1) & 1u); }

/* the CTB's own: NEW.  py, pcb, pcr: the 48 bin picks of each component (saostats::pick_bin; luma with lambda_luma and the luma M,
 * Cb and Cr with lambda_chroma and the chroma M; pcb, pcr not looked at without chroma).  Writes the triple and the whole record */
DBK_HD void new_ctb(const DbkSaoDecideArgs &a, int f, int cx, int cy, const saostats::BinPick *py, const saostats::BinPick *pcb,
                    const saostats::BinPick *pcr)
{
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    DbkSaoDecision r = {};
    DbkSaoCtb y, cb, cr;
    r.delta_d = saostats::pick_ctb(py, nullptr, a.lambda_luma, y, nullptr);
    r.cost_luma = saostats::pick_cost(py, nullptr, a.lambda_luma, y, nullptr);
    a.params_y[out] = y;
    if (a.stats_cb) {
        r.delta_d += saostats::pick_ctb(pcb, pcr, a.lambda_chroma, cb, &cr);
        r.cost_chroma = saostats::pick_cost(pcb, pcr, a.lambda_chroma, cb, &cr);
        a.params_cb[out] = cb;
        a.params_cr[out] = cr;
    }
    r.cand = (uint8_t)candidates(a, f, cx, cy);
    r.flag_bits = (uint8_t)flag_count(r.cand);
    a.decision[(long long)f * a.decision_frame_stride + (long long)cy * a.decision_stride + cx] = r;
}

/* NEW against LEFT against UP, in this order, the lowest J wins and on a tie the earliest.  The left and the upper CTB's triples in
 * params_* are FINAL when this runs; this CTB's own entries hold what new_ctb wrote */
DBK_HD void merge_ctb(const DbkSaoDecideArgs &a, int f, int cx, int cy)
{
    DbkSaoDecision &rec = a.decision[(long long)f * a.decision_frame_stride + (long long)cy * a.decision_stride + cx];
    const unsigned cand = rec.cand;
    if (!cand) return;
    const bool chroma = a.stats_cb != nullptr;
    const long long st = ((long long)f * a.stats_frame_stride + (long long)cy * a.stats_stride + cx) * saostats::kBins;
    const long long own = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    wide best = rd_cost(a, rec.cost_luma, rec.cost_chroma, flag_count(cand));
    DbkSaoDecision r = {};
    DbkSaoCtb y = {}, cb = {}, cr = {};
    for (unsigned m = kLeft; m <= kUp; m++) {
        if (!(cand & m)) continue;
        const long long from = m == kLeft ? own - 1 : own - a.params_stride;
        const DbkSaoCtb ny = a.params_y[from], ncb = chroma ? a.params_cb[from] : DbkSaoCtb{}, ncr = chroma ? a.params_cr[from] : DbkSaoCtb{};
        const long long dy = predicted(a.stats_y + st, ny), dc = chroma ? predicted(a.stats_cb + st, ncb) + predicted(a.stats_cr + st, ncr) : 0;
        const int bits = m == kLeft ? 1 : 1 + (int)(cand & kLeft);
        const wide j = rd_cost(a, 256 * dy, 256 * dc, bits);
        if (j < best) {
            best = j;
            y = ny; cb = ncb; cr = ncr;
            r.delta_d = dy + dc; r.cost_luma = 256 * dy; r.cost_chroma = 256 * dc;
            r.merge = (uint8_t)m; r.flag_bits = (uint8_t)bits;
        }
    }
    if (!r.merge) return;
    r.cand = (uint8_t)cand;
    a.params_y[own] = y;
    if (chroma) {
        a.params_cb[own] = cb;
        a.params_cr[own] = cr;
    }
    rec = r;
}

/* the anti-diagonal d = cx + cy of a grid: its first row and how many CTBs it has; CTB i of it is (d - (cy0 + i), cy0 + i) */
DBK_HD int diagonal(int ctbs_x, int ctbs_y, int d, int &cy0)
{
    cy0 = d < ctbs_x ? 0 : d - (ctbs_x - 1);
    const int cy1 = d < ctbs_y ? d : ctbs_y - 1;
    return cy1 - cy0 + 1;
}

} /* namespace saodecide */
