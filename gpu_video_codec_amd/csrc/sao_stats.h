/*
 * sao_stats.h -- SAO parameter estimation, the statistics pass: what one lane does with its 8x8 block of deblocked samples
 * (hevcdbk_sao_stats_device; the kernel around it is sao_stats.hip).  Every sample that is not kept is counted in its band bin and,
 * per edge class of Table 8-13, in the bin of its category when both neighbours of that class are available -- inside the plane and,
 * if in another CTB, not forbidden by the byte of the sample's own CTB.  That is exactly the condition under which
 * hevcdbk_sao_filter_device_nox would add offset[category - 1] to the sample.
 *
 * The procedure is written once, on functors: rows of samples come in through load functors, (bin, value) pairs leave through an
 * add functor -- LDS adds in the kernel, plain additions in tests/sao_stats_sim, which compiles this header for the CPU (DBK_HD, as
 * sao_packed.h does).  All arithmetic is 32-bit: one block adds at most 64 * 65535 to a bin.
 */
#pragma once
#include <stdint.h>

#include "deblock_packed.h" /* DBK_HD */
#include "sao_types.h"

/* the operands of the two launches (sao_stats.hip) as the host entries fill them (sao_stats_host.cpp).  Plain data */
struct DbkSaoStatsArgs {
    const uint8_t *rec, *org; /* the deblocked plane and the original, same geometry and container */
    long long rec_pitch, rec_frame_stride, org_pitch, org_frame_stride; /* bytes; a frame stride of 0 = shared */
    int plane_w, plane_h, n_frames, band_shift;
    int lw, lh; /* log2 of the CTB's width and height: 3..6, lh = lw or lw + 1 */
    const uint8_t *keep; /* may be NULL */
    int keep_stride;
    long long keep_frame_stride;
    const uint8_t *nox; /* may be NULL */
    int nox_stride;
    long long nox_frame_stride;
    int32_t *stats; /* 96 int32 per CTB */
    int stats_stride;
    long long stats_frame_stride; /* entries */
};
struct DbkSaoPickArgs {
    const int32_t *stats_a, *stats_b; /* stats_b NULL: one component */
    int stats_stride;
    long long stats_frame_stride;
    int ctbs_x, ctbs_y, n_frames;
    int max_offset; /* M = (1 << (Min(bitDepth, 10) - 5)) - 1 */
    long long lambda;
    DbkSaoCtb *params_a, *params_b;
    int params_stride;
    long long params_frame_stride;
    long long *delta_d; /* may be NULL; tight: [(f * ctbs_y + cy) * ctbs_x + cx] */
};

namespace saostats {

/* the bins of one CTB in the order of hevcdbk_sao_stats: eo_count[4][4], eo_sum[4][4], bo_count[32], bo_sum[32] */
constexpr int kBins = 96, kEoCount = 0, kEoSum = 16, kBoCount = 32, kBoSum = 64;

struct Geo {
    int w, h;       /* the plane, multiples of 4 */
    int lw, lh;     /* log2 of the CTB's width and height */
    int band_shift; /* bitDepth - 5 */
};

/* the bit of a CTB's byte that speaks for the neighbouring CTB (dcx, dcy), each negative / 0 / positive; (0, 0) = the CTB itself */
DBK_HD uint32_t nox_bit(int dcx, int dcy)
{
    return dcy < 0 ? (dcx < 0 ? 0x10u : (dcx > 0 ? 0x20u : 0x04u))
                   : (dcy > 0 ? (dcx < 0 ? 0x40u : (dcx > 0 ? 0x80u : 0x08u)) : (dcx < 0 ? 0x01u : (dcx > 0 ? 0x02u : 0u)));
}

/* sign(v): the median of (v, -1, 1), one instruction (written out: the compiler turns every plain form into two compares and two selects) */
DBK_HD int sgn(int v)
{
#if DBK_DEV
    int r;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(r) : "v"(v));
    return r;
#else
    return v < -1 ? -1 : (v > 1 ? 1 : v);
#endif
}

/*
 * Where the procedure adds: a CTB's working histogram of kSlots (count, sum) pairs -- per edge class FIVE slots indexed by
 * 2 + sign + sign (valley, corner, NONE, corner, peak), then the 32 bands.  The slot of a sample follows from its two signs by one
 * addition (count and sum: one address -- in the kernel one 64-bit LDS add); "none" -- a sample without a category, or with a neighbour that is not
 * available -- is a slot nobody adds to or reads.  bin_slot() maps the
 * 96 bins of hevcdbk_sao_stats onto the working histogram.
 */
constexpr int kSlots = 52, kBandSlot = 20;
DBK_HD int bin_slot(int bin) /* bin 0..95 in the order of hevcdbk_sao_stats -> below kSlots: the count of that slot; else the sum of slot - kSlots */
{
    const int sum = (bin >= kEoSum && bin < kBoCount) || bin >= kBoSum ? kSlots : 0;
    if (bin < kBoCount) {
        const int b = bin & 15, c = b & 3;
        return sum + (b >> 2) * 5 + c + (c >= 2);
    }
    return sum + kBandSlot + ((bin - kBoCount) & 31);
}

/* a block needs the per-sample availability test when it touches the plane's border or its CTB's byte forbids anything */
DBK_HD bool needs_check(const Geo &g, uint32_t nox, int x, int y0)
{
    return nox != 0u || x == 0 || y0 == 0 || x + 8 >= g.w || y0 + 8 >= g.h;
}

/*
 * The block at (x, y0), multiples of 8: 8 or 4 columns by 8 or 4 rows, the short ones being the last of a plane whose size is a
 * multiple of 4.  ld_rec(y, o): samples x-1 .. x+8 of the deblocked row y into o[0..9]; y is inside the plane or one row outside
 * (the functor clamps it), and positions outside the plane hold anything: CHECK discards what comes of them.  ld_org(y, o): samples
 * x .. x+7 of the original row.  add(slot, d): count[slot] += 1, sum[slot] += d in the working histogram of the block's CTB.
 * nox = the byte of the block's CTB (0: nothing forbidden).  CHECK = false is for blocks for which needs_check() is false: every
 * neighbour of every sample is available and the block is whole.
 */
template <bool CHECK, typename LoadRec, typename LoadOrg, typename Add>
DBK_HD void block(const Geo &g, uint32_t nox, int x, int y0, const LoadRec &ld_rec, const LoadOrg &ld_org, const Add &add)
{
    const int nc = !CHECK || x + 8 <= g.w ? 8 : g.w - x, nr = !CHECK || y0 + 8 <= g.h ? 8 : g.h - y0;
    int up[10], mid[10], dn[10];
    ld_rec(y0 - 1, up);
    ld_rec(y0, mid);
    for (int r = 0; r < nr; r++) {
        const int y = y0 + r;
        int og[8];
        ld_rec(y + 1, dn);
        ld_org(y, og);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (i < nc) {
                const int rec = mid[1 + i], d = og[i] - rec;
                add(kBandSlot + ((rec >> g.band_shift) & 31), d); /* & 31: a sample above the bit depth, a caller's error, stays inside */
#pragma unroll
                for (int k = 0; k < 4; k++) { /* Table 8-13: 0 (-1,0)/(1,0); 1 (0,-1)/(0,1); 2 (-1,-1)/(1,1); 3 (1,-1)/(-1,1) */
                    const int dxa = k == 1 ? 0 : (k == 3 ? 1 : -1), dya = k == 0 ? 0 : -1;
                    const int na = (dya ? up : mid)[1 + i + dxa], nb = (dya ? dn : mid)[1 + i - dxa];
                    int e = sgn(rec - na) + sgn(rec - nb); /* -2 valley, -1 / 1 corners, 2 peak, 0 none */
                    if constexpr (CHECK) {
                        const int xa = x + i + dxa, ya = y + dya, xb = x + i - dxa, yb = y - dya;
                        const int cx = (x + i) >> g.lw, cy = y >> g.lh;
                        const bool ok = xa >= 0 && xa < g.w && xb >= 0 && xb < g.w && ya >= 0 && ya < g.h && yb >= 0 && yb < g.h &&
                                        !(nox & (nox_bit((xa >> g.lw) - cx, (ya >> g.lh) - cy) | nox_bit((xb >> g.lw) - cx, (yb >> g.lh) - cy)));
                        e = ok ? e : 0;
                    }
                    if (e != 0) add(5 * k + 2 + e, d); /* a wave all of whose lanes have no category here -- smooth content -- skips the adds */
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 10; i++) {
            up[i] = mid[i];
            mid[i] = dn[i];
        }
    }
}

/* ---- from statistics to parameters (hevcdbk_sao_pick_device): the library's own rule, integers only ---------------------------- */

/* bits of an offset: |o| + 1, at most M (the truncated unary code of sao_offset_abs), and a sign bit for a non-zero band offset */
DBK_HD int offset_bits(int o, int M, bool band)
{
    const int a = o < 0 ? -o : o;
    return (a < M ? a + 1 : M) + (band && a ? 1 : 0);
}

/* the offset of a bin (n samples, sum s of org - rec): the rounded mean clamped to [lo, hi], then walked towards 0 while the cost
 * (n o^2 - 2 o s) * 256 + lambda * bits(o) does not rise: the least cost wins, on a tie the o nearer 0.  Returns o; cost out. */
DBK_HD int pick_offset(long long n, long long s, int lo, int hi, int M, bool band, long long lambda, long long &cost)
{
    if (n == 0) {
        cost = lambda * offset_bits(0, M, band);
        return 0;
    }
    const long long as = s < 0 ? -s : s;
    long long o0 = (2 * as + n) / (2 * n);
    if (s < 0) o0 = -o0;
    if (o0 < lo) o0 = lo;
    if (o0 > hi) o0 = hi;
    int best = (int)o0;
    long long best_cost = 0;
    for (long long o = o0;; o += o > 0 ? -1 : 1) {
        const long long c = (n * o * o - 2 * o * s) * 256 + lambda * offset_bits((int)o, M, band);
        if (o == o0 || c <= best_cost) {
            best = (int)o;
            best_cost = c;
        }
        if (o == 0) break;
    }
    cost = best_cost;
    return best;
}

/* the distortion change n o^2 - 2 o s of a chosen offset */
DBK_HD long long delta_d(long long n, long long s, int o) { return n * o * o - 2ll * o * s; }

/* the 48 bins a choice is made from, in the order of hevcdbk_sao_stats: 16 edge bins [class][category - 1], then 32 bands */
constexpr int kPickBins = 48;
struct BinPick {
    int o;
    long long cost, dd;
};
/* bin 0..47 of a CTB whose counts and sums are n[] / s[] as laid out in hevcdbk_sao_stats (int32 each: eo_count, eo_sum, bo_count,
 * bo_sum); M = (1 << (Min(bitDepth, 10) - 5)) - 1.  Edge categories 1, 2 take offsets 0..M, 3, 4 take -M..0 (7.4.9.3.2), bands -M..M */
DBK_HD BinPick pick_bin(const int32_t *st, int bin, int M, long long lambda)
{
    const bool band = bin >= 16;
    const long long n = band ? st[kBoCount + bin - 16] : st[kEoCount + bin], s = band ? st[kBoSum + bin - 16] : st[kEoSum + bin];
    const int lo = band ? -M : ((bin & 3) < 2 ? 0 : -M), hi = band ? M : ((bin & 3) < 2 ? M : 0);
    BinPick p;
    p.o = pick_offset(n, s, lo, hi, M, band, lambda, p.cost);
    p.dd = delta_d(n, s, p.o);
    return p;
}

/* the choice of a CTB from its bins' picks.  b == nullptr: one component -- "not applied" (lambda * 1), edge class 0..3 (lambda * 4
 * + its four bins), band position 0..31 (lambda * 7 + the four bands (p + k) & 31), in this order, the lowest cost wins and on a tie
 * the earliest.  With b (Cr beside Cb): one type and one edge class for both -- "not applied" (lambda * 1), edge class c (lambda * 4 +
 * both components' bins), band (lambda * 2 + per component lambda * 5 and its best position, the lowest on a tie).  Returns the
 * predicted change of the distortion, both components summed. */
DBK_HD long long pick_ctb(const BinPick *a, const BinPick *b, long long lambda, DbkSaoCtb &pa, DbkSaoCtb *pb)
{
    auto edge_cost = [](const BinPick *p, int c) { return p[4 * c].cost + p[4 * c + 1].cost + p[4 * c + 2].cost + p[4 * c + 3].cost; };
    auto band_cost = [](const BinPick *p, int pos) {
        return p[16 + (pos & 31)].cost + p[16 + ((pos + 1) & 31)].cost + p[16 + ((pos + 2) & 31)].cost + p[16 + ((pos + 3) & 31)].cost;
    };
    auto best_band = [&](const BinPick *p, long long &cost) {
        int pos = 0;
        cost = band_cost(p, 0);
        for (int q = 1; q < 32; q++) {
            const long long c = band_cost(p, q);
            if (c < cost) {
                cost = c;
                pos = q;
            }
        }
        return pos;
    };
    auto write = [](const BinPick *p, int type, int cls, DbkSaoCtb &out) {
        long long dd = 0;
        out.type = (uint8_t)type;
        out.cls = (uint8_t)cls;
        for (int k = 0; k < 4; k++) {
            const BinPick *q = type == 2 ? &p[4 * cls + k] : (type == 1 ? &p[16 + ((cls + k) & 31)] : nullptr);
            out.offset[k] = (int8_t)(q ? q->o : 0);
            dd += q ? q->dd : 0;
        }
        return dd;
    };
    long long best = lambda;
    int type = 0, cls = 0;
    for (int c = 0; c < 4; c++) {
        const long long cost = lambda * 4 + edge_cost(a, c) + (b ? edge_cost(b, c) : 0);
        if (cost < best) {
            best = cost;
            type = 2;
            cls = c;
        }
    }
    if (!b) {
        for (int pos = 0; pos < 32; pos++) {
            const long long cost = lambda * 7 + band_cost(a, pos);
            if (cost < best) {
                best = cost;
                type = 1;
                cls = pos;
            }
        }
        return write(a, type, cls, pa);
    }
    long long ca, cb;
    const int pos_a = best_band(a, ca), pos_b = best_band(b, cb);
    if (lambda * 12 + ca + cb < best) return write(a, 1, pos_a, pa) + write(b, 1, pos_b, *pb);
    return write(a, type, cls, pa) + write(b, type, cls, *pb);
}

/* the least cost pick_ctb found -- the cost of the candidate it wrote into pa (and *pb), by the same terms: what a caller needs who
 * weighs the choice against something else (sao_decide.h).  pa, pb: what pick_ctb(a, b, lambda, ...) gave */
DBK_HD long long pick_cost(const BinPick *a, const BinPick *b, long long lambda, const DbkSaoCtb &pa, const DbkSaoCtb *pb)
{
    auto four = [](const BinPick *p, const DbkSaoCtb &c) {
        long long cost = 0;
        for (int k = 0; k < 4; k++) cost += p[c.type == 2 ? 4 * c.cls + k : 16 + ((c.cls + k) & 31)].cost;
        return cost;
    };
    if (pa.type == 0) return lambda;
    if (pa.type == 2) return lambda * 4 + four(a, pa) + (b ? four(b, *pb) : 0);
    return b ? lambda * 12 + four(a, pa) + four(b, *pb) : lambda * 7 + four(a, pa);
}

} /* namespace saostats */
