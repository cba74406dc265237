/*
 * sao_slice_host.cpp -- C-ABI entries of slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation: hevcdbk_sao_decide_device_sf
 * (the decision under given flags), hevcdbk_sao_slice_flags_device (the flags chosen per slice, and the decision under them) and
 * hevcdbk_sao_slice_flags_workspace.  The checks are the decision's one list (sao_decide_host.cpp).  Kernels: sao_slice.hip.
 */
#include "deblock_ctx.h"
#include "sao_decide_host.h"
#include "sao_slice_launch.h"

extern "C" {

size_t hevcdbk_sao_slice_flags_workspace(unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned n_slices)
{
    (void)n_slices; /* the sums per slice live in LDS */
    return ((size_t)saoslice::kStateBytes * ctbs_x * ctbs_y * n_frames + 15) & ~(size_t)15;
}

int hevcdbk_sao_decide_device_sf(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                 const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x,
                                 unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma, unsigned bit_depth_chroma,
                                 unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma, unsigned lambda_q8_luma,
                                 unsigned lambda_q8_chroma, const uint16_t *slice_idx, const uint16_t *tile_idx, unsigned idx_stride,
                                 size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr,
                                 unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                 size_t decision_frame_stride, const uint8_t *slice_flags, unsigned n_slices, size_t slice_flags_frame_stride,
                                 void *hip_stream)
{
    const unsigned scale[2] = {log2_offset_scale_luma, log2_offset_scale_chroma};
    DbkSaoSliceOps so = {};
    so.n_slices = n_slices;
    so.flags_frame_stride = slice_flags_frame_stride;
    so.flags_in = slice_flags;
    return dbk_sao_decide_entry(ctx, stats_y, stats_cb, stats_cr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth_luma,
                                bit_depth_chroma, scale, lambda_q8_luma, lambda_q8_chroma, slice_idx, tile_idx, idx_stride, idx_frame_stride, params_y,
                                params_cb, params_cr, params_stride, params_frame_stride, decision, decision_stride, decision_frame_stride,
                                slice_flags ? &so : nullptr, hip_stream); /* no flags: hevcdbk_sao_decide_device_os itself */
}

int hevcdbk_sao_slice_flags_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                   const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x,
                                   unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma, unsigned bit_depth_chroma,
                                   unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma, unsigned lambda_q8_luma,
                                   unsigned lambda_q8_chroma, const uint16_t *slice_idx, const uint16_t *tile_idx, unsigned idx_stride,
                                   size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr,
                                   unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                   size_t decision_frame_stride, unsigned n_slices, uint8_t *slice_flags, size_t slice_flags_frame_stride,
                                   hevcdbk_sao_slice_record *slice_record, size_t slice_record_frame_stride, void *workspace,
                                   size_t workspace_bytes, void *hip_stream)
{
    const unsigned scale[2] = {log2_offset_scale_luma, log2_offset_scale_chroma};
    DbkSaoSliceOps so = {};
    so.choose = true;
    so.n_slices = n_slices;
    so.flags_frame_stride = slice_flags_frame_stride;
    so.flags_out = slice_flags;
    so.record = slice_record;
    so.record_frame_stride = slice_record_frame_stride;
    so.workspace = workspace;
    so.workspace_bytes = workspace_bytes;
    return dbk_sao_decide_entry(ctx, stats_y, stats_cb, stats_cr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth_luma,
                                bit_depth_chroma, scale, lambda_q8_luma, lambda_q8_chroma, slice_idx, tile_idx, idx_stride, idx_frame_stride, params_y,
                                params_cb, params_cr, params_stride, params_frame_stride, decision, decision_stride, decision_frame_stride, &so,
                                hip_stream);
}

} /* extern "C" */
