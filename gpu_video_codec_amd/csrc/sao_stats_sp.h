/*
 * sao_stats_sp.h -- SAO parameter estimation on a semi-planar chroma plane (interleaved Cb / Cr pairs): how one lane reads the rows
 * of ONE component of its 8x8 block of pairs (hevcdbk_sao_stats_device_sp; the kernel around it is sao_stats_sp.hip).  The rule is
 * that of sao_stats.h per component -- saostats::block runs unchanged on the loaders below -- with every coordinate counted in
 * PAIRS: the neighbour of a sample is the neighbouring pair's sample of the same component, never the adjacent sample of the row.
 *
 * Everything that decides WHICH BYTES are touched -- the row clamp on rows -1 and h, the left and right halo pair, the 4-pair last
 * block -- is here, DBK_HD, and tests/sao_stats_sp_sim compiles exactly this for the CPU with every operand in a heap block of its
 * own size.  No load touches a byte outside pitch * plane_h of a frame: a wide load covers pairs q .. q + 3 with q + 4 <= w, a
 * narrow one the sample 2 * p + c with p < w, and 2 * w samples fit in a pitch.
 */
#pragma once
#include <stdint.h>

#include "sao_stats.h"

/* the operands of the launch (sao_stats_sp.hip) as the host entry fills them (sao_stats_host.cpp): those of the planar launch with
 * plane_w x plane_h counted per component and lw = lh; p.stats is Cb's array (the even samples), stats_cr Cr's, one stride for both */
struct DbkSaoStatsSpArgs {
    DbkSaoStatsArgs p;
    int32_t *stats_cr;
};

namespace saostats_sp {

/* one frame of a pair plane: w x h pairs, rows `pitch` bytes apart */
struct Plane {
    const uint8_t *base;
    long long pitch;
    int w, h;
};

/* the row a load of row y (inside the plane, or one row outside it) reads */
DBK_HD int row_of(int y, int h) { return y < 0 ? 0 : (y >= h ? h - 1 : y); }

/* The four wide loads of a block at pair x (a multiple of 8, x < w; w a multiple of 4): the first pair of each.  Left half, right
 * half (the 4-pair last block has none: its left half again, never used), the quad whose LAST pair is the left halo (x - 1; at
 * x = 0 the first quad, discarded by CHECK), the quad whose FIRST pair is the right halo (x + 8; past the plane the last quad) */
DBK_HD int quad_lo(int x) { return x; }
DBK_HD int quad_hi(int x, int w) { return x + 8 <= w ? x + 4 : x; }
DBK_HD int quad_left(int x) { return x >= 4 ? x - 4 : 0; }
DBK_HD int quad_right(int x, int w) { return x + 12 <= w ? x + 8 : w - 4; }
/* sample by sample: the pair read for position p of the row */
DBK_HD int pair_of(int p, int w) { return p < 0 ? 0 : (p >= w ? w - 1 : p); }

template <typename T>
struct Quad;
template <>
struct Quad<uint8_t> { /* 8 bytes: Cb0 Cr0 Cb1 Cr1 | Cb2 Cr2 Cb3 Cr3 */
    static constexpr int kWords = 2;
    static DBK_HD void pick(const uint32_t (&v)[2], int c, int *o)
    {
        const int s = 8 * c;
        o[0] = (v[0] >> s) & 0xff; o[1] = (v[0] >> (16 + s)) & 0xff; o[2] = (v[1] >> s) & 0xff; o[3] = (v[1] >> (16 + s)) & 0xff;
    }
};
template <>
struct Quad<uint16_t> { /* 16 bytes: one pair per word */
    static constexpr int kWords = 4;
    static DBK_HD void pick(const uint32_t (&v)[4], int c, int *o)
    {
        const int s = 16 * c;
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = (v[i] >> s) & 0xffff;
    }
};

/* component c of the four pairs q .. q + 3 of a row whose first byte is a multiple of 8 * sizeof(T): one load of 8 samples */
template <typename T>
DBK_HD void ld_quad(const uint8_t *row, int q, int c, int *o)
{
    constexpr int N = Quad<T>::kWords;
    uint32_t v[N];
    __builtin_memcpy(v, __builtin_assume_aligned(row + (size_t)q * 2 * sizeof(T), 4 * N), 4 * N);
    Quad<T>::pick(v, c, o);
}

/* saostats::block's ld_rec: component c of pairs x - 1 .. x + 8 of the deblocked row y into o[0..9] */
template <typename T, bool VEC>
DBK_HD void ld_rec(const Plane &p, int c, int x, int y, int (&o)[10])
{
    const uint8_t *row = p.base + (long long)row_of(y, p.h) * p.pitch;
    if constexpr (VEC) {
        int l[4], r[4];
        ld_quad<T>(row, quad_lo(x), c, &o[1]);
        ld_quad<T>(row, quad_hi(x, p.w), c, &o[5]);
        ld_quad<T>(row, quad_left(x), c, l);
        ld_quad<T>(row, quad_right(x, p.w), c, r);
        o[0] = l[3];
        o[9] = r[0];
    } else {
        const T *s = reinterpret_cast<const T *>(row);
#pragma unroll
        for (int i = 0; i < 10; i++) o[i] = s[2 * pair_of(x - 1 + i, p.w) + c];
    }
}

/* saostats::block's ld_org: component c of pairs x .. x + 7 of the original row y (inside the plane) */
template <typename T, bool VEC>
DBK_HD void ld_org(const Plane &p, int c, int x, int y, int (&o)[8])
{
    const uint8_t *row = p.base + (long long)y * p.pitch;
    if constexpr (VEC) {
        ld_quad<T>(row, quad_lo(x), c, &o[0]);
        ld_quad<T>(row, quad_hi(x, p.w), c, &o[4]);
    } else {
        const T *s = reinterpret_cast<const T *>(row);
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = s[2 * pair_of(x + i, p.w) + c];
    }
}

/* the frame f of a plane whose frames are frame_stride bytes apart (0: one frame for all) */
DBK_HD Plane frame_of(const uint8_t *base, long long pitch, long long frame_stride, int f, int w, int h)
{
    return Plane{base + (long long)f * frame_stride, pitch, w, h};
}

/* the keep byte of the block at pair (x, y0): one byte per 8x8 PAIRS, for both components */
DBK_HD long long keep_at(int x, int y0, int keep_stride, long long keep_frame_stride, int f)
{
    return (long long)f * keep_frame_stride + (long long)(y0 >> 3) * keep_stride + (x >> 3);
}
/* the borders byte of the block's CTB: one byte per CTB of the per-component grid, for both components */
DBK_HD long long nox_at(int x, int y0, int lg, int nox_stride, long long nox_frame_stride, int f)
{
    return (long long)f * nox_frame_stride + (long long)(y0 >> lg) * nox_stride + (x >> lg);
}

} /* namespace saostats_sp */
