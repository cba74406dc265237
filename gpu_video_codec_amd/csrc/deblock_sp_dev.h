/* deblock_sp_dev.h -- device side of the semi-planar chroma kernels: the operand fetch of a lane's offset block of sample PAIRS, shared by
 * the deblocking kernels (deblock_sp.hip) and the fused deblocking + SAO kernels (deblock_sao_sp_fused.h). */
#pragma once
#include "deblock_h265.h"
#include "deblock_sl_dev.h"
#include "deblock_sl_packed.h"

namespace dbk {

/* what the two components of a lane's block share: the four bS bytes, the four segment QPs and the four offset pairs (the launch's
 * own pair added).  Every load is issued before anything waits. */
__device__ __forceinline__ void sp_block_operands(const DbkH265Args &h, const DbkSlOffs &sl, int f, int bx, int by, int (&entry)[4],
                                                  int (&qpl)[4], int (&tc_off)[4], int (&beta_off)[4])
{
    const DbkArgs &a = h.base;
    unsigned ar, bl, br;
    dbk_sl_load_pairs<2, 2>(sl, f, bx, by, a.plane_w * 2, a.plane_h * 2, ar, bl, br);
    dbk::load_block_bs_h265_g4(a.vert_bs + (long long)f * a.vert_bs_stride, a.hor_bs + (long long)f * a.hor_bs_stride, bx, by,
                               a.plane_w, a.plane_h, a.vstride, a.hstride, entry);
    if (a.qp_map) { /* wave-uniform */
        dbk::h265_block_qpl4(a.qp_map + (long long)f * a.map_frame_stride, a.map_stride, a.ctu_log2, 2, a.plane_w * 2, a.plane_h * 2,
                             bx * 8 - 4, by * 8 - 4, qpl);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) qpl[i] = h.qp;
    }
    dbk::h265_sl_seg_offs(ar, bl, br, tc_off, beta_off);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        tc_off[i] += h.tc_off;
        beta_off[i] += h.beta_off;
    }
}

/* the two components' per-segment operands from what they share */
__device__ __forceinline__ void sp_seg_params(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int f, int bx, int by, int shift,
                                              int max_v, dbk::H265Seg &cb, dbk::H265Seg &cr)
{
    int entry[4], qpl[4], tc_off[4], beta_off[4];
    sp_block_operands(h, sl, f, bx, by, entry, qpl, tc_off, beta_off);
    const dbk::H265Prm pb = {0, 0, h.c_qp_offset, shift, max_v}, pr = {0, 0, cr_qp_offset, shift, max_v};
    dbk::h265_seg_params_sl<true, 1>(entry, qpl, pb, tc_off, beta_off, cb);
    dbk::h265_seg_params_sl<true, 1>(entry, qpl, pr, tc_off, beta_off, cr);
}

} /* namespace dbk */
