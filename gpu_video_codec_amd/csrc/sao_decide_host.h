/* sao_decide_host.h -- PRIVATE to the library: the one list of checks of the SAO decision's entries (sao_decide_host.cpp), as the
 * entries of sao_slice_host.cpp call it */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hevc_deblock.h"

/* what the entries with slice-level flags add to the operands of hevcdbk_sao_decide_device_os */
struct DbkSaoSliceOps {
    bool choose;                      /* false: hevcdbk_sao_decide_device_sf; true: hevcdbk_sao_slice_flags_device */
    unsigned n_slices;
    size_t flags_frame_stride;
    const uint8_t *flags_in;          /* the decision under given flags: not NULL */
    uint8_t *flags_out;               /* the choice */
    hevcdbk_sao_slice_record *record; /* may be NULL */
    size_t record_frame_stride;
    void *workspace;
    size_t workspace_bytes;
};

/* scale == nullptr: hevcdbk_sao_decide_device; so == nullptr: no slice-level flags (so needs scale) */
int dbk_sao_decide_entry(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb, const hevcdbk_sao_stats *stats_cr,
                         unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                         unsigned bit_depth_chroma, const unsigned *scale, unsigned lambda_q8_luma, unsigned lambda_q8_chroma, const uint16_t *slice_idx,
                         const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb,
                         hevcdbk_sao_ctb *params_cr, unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision,
                         unsigned decision_stride, size_t decision_frame_stride, const DbkSaoSliceOps *so, void *hip_stream);
