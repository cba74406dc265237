/* deblock_sl_dev.h -- device side of the per-slice deblocking offsets (deblock_sl.h): the loads of a lane's three pairs, shared
 * by the 32-bit kernels (deblock_sl.hip) and the packed / fused kernels (deblock_kernels.hip). */
#pragma once
#include "deblock_kernels.h"
#include "deblock_sl.h"

/* the words of the three CTBs of block (bx, by) of a plane with SubWidthC x SubHeightC = SX x SY: above-right, below-left,
 * below-right.  Each pair is ONE 16-bit load through a buffer resource whose range is the frame's array itself (sl.n_bytes), so an
 * offset beyond it reads 0 and never memory; the offsets come from 24-bit multiplies (2 * stride and the CTB row are far below
 * 2^24: the entry points check); f * frame_stride in 64 bits (a batch's arrays may lie gigabytes apart).  No wait in here. */
template <int SX, int SY>
__device__ __forceinline__ void dbk_sl_load_pairs(const DbkSlOffs &sl, int f, int bx, int by, int lw, int lh, unsigned &ar, unsigned &bl,
                                                  unsigned &br)
{
    int cx[2], cy[2];
    dbk::h265_sl_ctbs<SX, SY>(bx, by, lw, lh, sl.ctb_log2, cx, cy);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<int8_t *>(sl.offs) + (long long)f * sl.frame_stride, 0, sl.n_bytes, 0x00020000);
    const uint32_t row2 = (uint32_t)sl.stride * 2u;
    const uint32_t ot = __umul24((uint32_t)cy[0], row2), ob = __umul24((uint32_t)cy[1], row2);
    ar = __builtin_amdgcn_raw_buffer_load_b16(rs, ot + 2u * (uint32_t)cx[1], 0, 0);
    bl = __builtin_amdgcn_raw_buffer_load_b16(rs, ob + 2u * (uint32_t)cx[0], 0, 0);
    br = __builtin_amdgcn_raw_buffer_load_b16(rs, ob + 2u * (uint32_t)cx[1], 0, 0);
}
