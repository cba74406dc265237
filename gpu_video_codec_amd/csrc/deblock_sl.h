/*
 * deblock_sl.h -- per-slice deblocking offsets of the SPEC-EXACT mode (hevcdbk_h265_slice_offsets of the C ABI).
 *
 * H.265 8.7.2.5.3 (luma) and 8.7.2.5.5 (chroma) take slice_beta_offset_div2 / slice_tc_offset_div2 from the slice that holds
 * sample q0,0 of the edge segment.  Slices are made of whole CTBs of at least 16 luma samples and edges lie on the 8-sample grid,
 * so one pair per CTB of the LUMA grid is exact for every plane: a chroma plane finds its CTB at luma (x * SubWidthC,
 * y * SubHeightC).
 *
 * The q0,0 samples of an offset block's four segments (block centre = plane sample (8 bx, 8 by)):
 *   ver1 (8 bx, 8 by - 4)   above-right of the centre
 *   ver2 (8 bx, 8 by)       below-right
 *   hor1 (8 bx - 4, 8 by)   below-left
 *   hor2 (8 bx, 8 by)       below-right (the conformant hor2: columns 4..7)
 * i.e. three CTBs at most, out of two CTB columns and two CTB rows.
 *
 * DBK_HD like deblock_h265.h: tests/sl_sim runs this rule and the block filter on the CPU against tests/slice_offsets_ref.py.
 */
#pragma once
#include "deblock_h265.h"

namespace dbk {

/* CTB columns (left, right) and rows (top, bottom) of the luma grid that hold the block's q0,0 samples; SX / SY = SubWidthC /
 * SubHeightC of the plane (1 / 1 for luma); lw / lh = the luma picture size.  Positions outside the picture (the halves of
 * frame-edge blocks, whose bS entries are 0 anyway) are clamped into it, so every index is inside the array. */
template <int SX, int SY>
DBK_HD void h265_sl_ctbs(int bx, int by, int lw, int lh, int ctb_log2, int (&cx)[2], int (&cy)[2])
{
    cx[0] = clampi((bx * 8 - 4) * SX, 0, lw - 1) >> ctb_log2;
    cx[1] = clampi((bx * 8) * SX, 0, lw - 1) >> ctb_log2;
    cy[0] = clampi((by * 8 - 4) * SY, 0, lh - 1) >> ctb_log2;
    cy[1] = clampi((by * 8) * SY, 0, lh - 1) >> ctb_log2;
}

/* a pair as one 16-bit word (offs[2 i] = beta in the low byte, offs[2 i + 1] = tc in the high byte) -> the doubled offsets
 * H265Prm carries (slice_*_offset_div2 << 1) */
DBK_HD int h265_sl_beta_off(unsigned pair) { return (int)(int8_t)(pair & 0xffu) * 2; }
DBK_HD int h265_sl_tc_off(unsigned pair) { return (int)(int8_t)((pair >> 8) & 0xffu) * 2; }

/* the pairs of the block's four segments (ver1, ver2, hor1, hor2) from the three CTBs' words: ar = above-right, bl = below-left,
 * br = below-right */
DBK_HD void h265_sl_seg_offs(unsigned ar, unsigned bl, unsigned br, int (&tc_off)[4], int (&beta_off)[4])
{
    const unsigned w[4] = {ar, br, bl, br};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        tc_off[i] = h265_sl_tc_off(w[i]);
        beta_off[i] = h265_sl_beta_off(w[i]);
    }
}

/* filter_block_h265 / filter_block_h265_chroma_cf with offsets per segment; CF 0 = luma, 1..3 = a chroma plane of that format.
 * p.tc_off / p.beta_off are not used. */
template <int CF>
DBK_HD void filter_block_h265_sl(int (&v)[8][8], const int (&entry)[4], const int (&qpl)[4], const H265Prm &p, const int (&tc_off)[4],
                                 const int (&beta_off)[4])
{
    H265Prm q[4] = {p, p, p, p};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        q[i].tc_off = tc_off[i];
        q[i].beta_off = beta_off[i];
    }
    if constexpr (CF == 0) {
        h265_luma_segment<SegVer1>(v, entry[0], qpl[0], q[0]);
        h265_luma_segment<SegVer2>(v, entry[1], qpl[1], q[1]);
        h265_luma_segment<SegHor1>(v, entry[2], qpl[2], q[2]);
        h265_luma_segment<SegHor2S>(v, entry[3], qpl[3], q[3]);
    } else {
        h265_chroma_segment_cf<SegVer1, CF>(v, entry[0], qpl[0], q[0]);
        h265_chroma_segment_cf<SegVer2, CF>(v, entry[1], qpl[1], q[1]);
        h265_chroma_segment_cf<SegHor1, CF>(v, entry[2], qpl[2], q[2]);
        h265_chroma_segment_cf<SegHor2S, CF>(v, entry[3], qpl[3], q[3]);
    }
}

} /* namespace dbk */
