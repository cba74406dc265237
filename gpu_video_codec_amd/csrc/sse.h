/*
 * sse.h -- measured distortion: what one lane does with its block of a plane and of the original (hevcdbk_sse_device,
 * hevcdbk_sse_device_sp; the kernels around it are in sse.hip), and how the lanes of a wave add their blocks up to CTBs.  Exact
 * integers: a lane sums the squares of (org - rec) over the samples of its block that lie inside the plane, a CTB's sum is a
 * butterfly over the lanes of that CTB, 64 bits wide.
 *
 * A lane owns 8 rows of NS samples: NS = 8 (one 8x8 block), or 16 as two sums -- the two 8x8 blocks side by side of an 8-bit plane
 * on the 16-byte path (kHalves), or the 8x8 pairs of a plane of interleaved Cb / Cr pairs (kParity: even samples, odd samples).
 * Three ways to fetch a row piece, all giving the same bytes and none touching a byte outside plane_w x plane_h samples:
 *   kWide    16 bytes per load where 16 bytes lie inside the plane, four samples per load for what is left of a ragged piece
 *   kQuad    four samples per load
 *   kScalar  sample by sample
 * Everything here is DBK_HD: tests/sse_sim compiles it for the CPU and runs it lane by lane, butterfly step by butterfly step.
 */
#pragma once
#include <stdint.h>

#include "deblock_packed.h" /* DBK_HD */

/* the operands of the two launches (sse.hip) as the host entries fill them (sse_host.cpp).  Plain data */
struct DbkSseArgs {
    const uint8_t *rec, *org; /* the plane and the original, same geometry and container */
    long long rec_pitch, rec_frame_stride, org_pitch, org_frame_stride; /* bytes; a frame stride of 0 = shared */
    int plane_w, plane_h, n_frames; /* a pair plane: per component */
    int lw, lh;                     /* log2 of the CTB's width and height: 3..6, lh = lw or lw + 1 */
    int wide_acc;                   /* bit depth above 13: 64 squares of a lane do not fit 32 bits */
    unsigned long long *sse;        /* one per CTB; a pair plane: the even samples' */
    unsigned long long *sse_odd;    /* a pair plane: the odd samples'; else NULL */
    int sse_stride;
    long long sse_frame_stride; /* entries */
};
struct DbkSseTotalsArgs {
    const unsigned long long *sse;
    int sse_stride;
    long long sse_frame_stride;
    int ctbs_x, ctbs_y, n_frames;
    const uint16_t *slice_idx; /* may be NULL: every CTB in slice 0 */
    int idx_stride;
    long long idx_frame_stride;
    int n_slices; /* 1..kMaxSlices */
    unsigned long long *slice_total; /* may be NULL */
    long long slice_total_frame_stride;
    unsigned long long *frame_total; /* may be NULL */
};

namespace sse {

constexpr int kScalar = 0, kQuad = 1, kWide = 2;  /* how a row piece is fetched */
constexpr int kOne = 0, kHalves = 1, kParity = 2; /* which of a lane's two sums sample i of a row piece goes to */
constexpr int kMaxSlices = 600;                   /* the totals of a frame live in LDS */
constexpr int kAcc32MaxDepth = 13;                /* 64 * 8191^2 < 2^32 <= 64 * 16383^2 */

/* (org - rec)^2, |d| <= 65535: the product fits 32 bits.  Both factors are the difference of two samples the loaders have masked to
 * 16 bits, which the compiler sees: it takes the 24-bit multiplier (v_mad_i32_i24 / v_mul_i32_i24, full rate) on its own */
DBK_HD uint32_t sq(int d) { return (uint32_t)d * (uint32_t)d; }

template <typename T>
DBK_HD int sample_of(const uint32_t *v, int i)
{
    if constexpr (sizeof(T) == 1) return (int)((v[i >> 2] >> (8 * (i & 3))) & 0xffu);
    else return (int)((v[i >> 1] >> (16 * (i & 1))) & 0xffffu);
}

/* samples 0 .. n - 1 (n a multiple of 4, at most NS) of the row piece at p into o[], 0 into the rest; FULL: n == NS, no conditions.
 * kWide: a 16-byte chunk that lies wholly inside the piece is one load, what is left of a ragged piece comes in quads */
template <typename T, int MODE, int NS, bool FULL>
DBK_HD void load_row(const uint8_t *p, int n, int (&o)[NS])
{
    constexpr int kQuadBytes = 4 * (int)sizeof(T), kChunk = 16 / (int)sizeof(T); /* samples in 16 bytes */
    if constexpr (MODE == kScalar) {
        const T *s = reinterpret_cast<const T *>(p);
#pragma unroll
        for (int i = 0; i < NS; i++) o[i] = FULL || i < n ? (int)s[i] : 0;
    } else if constexpr (MODE == kQuad) {
#pragma unroll
        for (int q = 0; q < NS / 4; q++) {
            uint32_t v[sizeof(T)] = {};
            if (FULL || 4 * q < n) __builtin_memcpy(v, __builtin_assume_aligned(p + q * kQuadBytes, kQuadBytes), kQuadBytes);
#pragma unroll
            for (int i = 0; i < 4; i++) o[4 * q + i] = sample_of<T>(v, i);
        }
    } else {
        static_assert(NS % kChunk == 0, "a wide row piece is whole 16-byte chunks");
#pragma unroll
        for (int c = 0; c < NS / kChunk; c++) {
            uint32_t v[4] = {};
            if (FULL || (c + 1) * kChunk <= n) {
                __builtin_memcpy(v, __builtin_assume_aligned(p + c * 16, 16), 16);
            } else {
#pragma unroll
                for (int q = 0; q < kChunk / 4; q++)
                    if (c * kChunk + 4 * q < n)
                        __builtin_memcpy(v + q * (int)sizeof(T), __builtin_assume_aligned(p + c * 16 + q * kQuadBytes, kQuadBytes), kQuadBytes);
            }
#pragma unroll
            for (int i = 0; i < kChunk; i++) o[c * kChunk + i] = sample_of<T>(v, i);
        }
    }
}

/*
 * The sums of one lane: rows 0 .. m - 1 (m = 4 or 8) of n samples (a multiple of 4, at most NS) at rec / org.  Acc = uint32_t where
 * 64 squares fit (depths up to kAcc32MaxDepth), else uint64_t.  FULL: n == NS and m == 8, no conditions.
 */
template <typename T, int MODE, int NS, int SPLIT, bool FULL, typename Acc>
DBK_HD void block_sums(const uint8_t *rec, const uint8_t *org, long long rec_pitch, long long org_pitch, int n, int m, Acc (&s)[2])
{
    s[0] = s[1] = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (!FULL && r >= m) break;
        int a[NS], b[NS];
        load_row<T, MODE, NS, FULL>(rec + r * rec_pitch, n, a);
        load_row<T, MODE, NS, FULL>(org + r * org_pitch, n, b);
#pragma unroll
        for (int i = 0; i < NS; i++) {
            const int k = SPLIT == kHalves ? i >> 3 : (SPLIT == kParity ? i & 1 : 0);
            if (FULL || i < n) s[k] += (Acc)sq(b[i] - a[i]);
        }
    }
}

/*
 * From blocks to CTBs.  Lane by * 8 + bx of a wave holds the sum of the block (bx, by) of the wave's region.  hsteps horizontal
 * steps (partner lane ^ 1, ^ 2, ^ 4) and vsteps vertical ones (^ 8, ^ 16, ^ 32) leave in EVERY lane the sum of the aligned
 * 2^hsteps x 2^vsteps group of blocks it belongs to; integer adds commute, so the order of the steps changes no bit.  A CTB of
 * 2^lw x 2^lh samples over blocks of 2^bw_log2 x 8: hsteps = lw - bw_log2 (0 where a lane is as wide as a CTB or wider),
 * vsteps = lh - 3.  The lane that stores is the group's first.
 */
DBK_HD int h_steps(int lw, int bw_log2) { return lw > bw_log2 ? lw - bw_log2 : 0; }
DBK_HD int v_steps(int lh) { return lh - 3; }
DBK_HD int step_mask(int i, int hsteps) { return i < hsteps ? 1 << i : 8 << (i - hsteps); }
DBK_HD bool stores(int lane, int hsteps, int vsteps) { return ((lane & 7) & ((1 << hsteps) - 1)) == 0 && ((lane >> 3) & ((1 << vsteps) - 1)) == 0; }

/* xchg(v, mask): the value v of lane ^ mask */
template <typename Xchg>
DBK_HD unsigned long long butterfly(unsigned long long v, int hsteps, int vsteps, const Xchg &xchg)
{
    for (int i = 0; i < hsteps + vsteps; i++) v += xchg(v, step_mask(i, hsteps));
    return v;
}

/* Before the butterfly: a lane that holds two 8x8 blocks side by side (kHalves) holds two CTBs only where CTBs are 8 wide; else the
 * two are one CTB's.  two_sums: both of a lane's sums go through the butterfly */
template <int SPLIT>
DBK_HD bool two_sums(int lw) { return SPLIT == kParity || (SPLIT == kHalves && lw == 3); }
template <int SPLIT>
DBK_HD void fold(int lw, unsigned long long (&s)[2])
{
    if (SPLIT == kHalves && lw != 3) {
        s[0] += s[1];
        s[1] = 0;
    }
}

/* After the butterfly: what the lane `lane` of the region at (rx, ry), blocks bw wide, stores.  store(which, cx, cy, v): which = 0 the
 * array of the plane / of the even samples, 1 that of the odd samples.  One lane per CTB of the grid, nothing beyond the grid */
template <int SPLIT, typename Store>
DBK_HD void store_ctbs(int lane, int rx, int ry, int bw, int w, int h, int lw, int lh, int hsteps, int vsteps, const unsigned long long (&s)[2],
                       const Store &store)
{
    if (!stores(lane, hsteps, vsteps)) return;
    const int ctbs_x = (w + (1 << lw) - 1) >> lw, ctbs_y = (h + (1 << lh) - 1) >> lh;
    const int cx = (rx + (lane & 7) * bw) >> lw, cy = (ry + (lane >> 3) * 8) >> lh;
    if (cx >= ctbs_x || cy >= ctbs_y) return;
    store(0, cx, cy, s[0]);
    if (SPLIT == kParity) store(1, cx, cy, s[1]);
    else if (SPLIT == kHalves && lw == 3 && cx + 1 < ctbs_x) store(0, cx + 1, cy, s[1]);
}

/* the geometry of a lane's block: where it lies, and what of it is inside the plane */
struct Block {
    int x, y0; /* first sample (a pair plane: pair) and row */
    int n, m;  /* samples (pairs) and rows inside the plane; 0 = wholly outside */
};
DBK_HD Block block_of(int region_x, int region_y, int lane, int bw, int w, int h)
{
    Block b;
    b.x = region_x + (lane & 7) * bw;
    b.y0 = region_y + (lane >> 3) * 8;
    b.n = b.x < w && b.y0 < h ? (w - b.x < bw ? w - b.x : bw) : 0;
    b.m = b.n ? (h - b.y0 < 8 ? h - b.y0 : 8) : 0;
    return b;
}

/*
 * One lane of the planar kernel: the block's one or two sums (kHalves: NS == 16, the left and the right 8 columns), 64 bits wide.
 * rec / org: the frame's first byte.
 */
template <typename T, int MODE, int NS, int SPLIT, typename Acc>
DBK_HD void lane_sums(const uint8_t *rec, const uint8_t *org, long long rec_pitch, long long org_pitch, const Block &b, int samples_per_unit,
                      unsigned long long (&out)[2])
{
    out[0] = out[1] = 0;
    if (b.n == 0) return;
    const size_t at = (size_t)b.x * samples_per_unit * sizeof(T);
    const uint8_t *r = rec + (long long)b.y0 * rec_pitch + at, *o = org + (long long)b.y0 * org_pitch + at;
    Acc s[2];
    const int n = b.n * samples_per_unit;
    if (n == NS && b.m == 8) block_sums<T, MODE, NS, SPLIT, true, Acc>(r, o, rec_pitch, org_pitch, n, b.m, s);
    else block_sums<T, MODE, NS, SPLIT, false, Acc>(r, o, rec_pitch, org_pitch, n, b.m, s);
    out[0] = s[0];
    out[1] = s[1];
}

/*
 * The totals of one frame (hevcdbk_sse_totals_device): a lane walks its CTBs in raster order and keeps the running sum of the slice
 * it is in; flush(slice, sum) adds it to the frame's array when the slice changes and at the end.  Slices are runs in raster
 * order, so a lane flushes about once per slice it meets, not once per CTB.  Returns the lane's share of the frame total.
 */
template <typename Flush>
DBK_HD unsigned long long totals_walk(const unsigned long long *sse, int sse_stride, const uint16_t *idx, int idx_stride, int ctbs_x, int ctbs_y,
                                      int n_slices, int row0, int row_step, int col0, int col_step, const Flush &flush)
{
    unsigned long long all = 0, run = 0;
    int cur = -1;
    for (int cy = row0; cy < ctbs_y; cy += row_step)
        for (int cx = col0; cx < ctbs_x; cx += col_step) {
            const unsigned long long v = sse[(long long)cy * sse_stride + cx];
            all += v;
            const int s = idx ? (int)idx[(long long)cy * idx_stride + cx] : 0;
            if (s != cur) {
                if (cur >= 0 && cur < n_slices) flush(cur, run);
                cur = s;
                run = 0;
            }
            run += v;
        }
    if (cur >= 0 && cur < n_slices) flush(cur, run);
    return all;
}

} /* namespace sse */
