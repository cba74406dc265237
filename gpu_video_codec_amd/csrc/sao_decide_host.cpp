/*
 * sao_decide_host.cpp -- C-ABI entries of the SAO decision per CTB: hevcdbk_sao_decide_device (own parameters, merge left or merge up
 * over Y, Cb and Cr from the statistics of hevcdbk_sao_stats_device / _sp) and hevcdbk_sao_decide_device_os (the same with
 * log2_sao_offset_scale_luma / _chroma); and the one list of checks they share with the entries of sao_slice_host.cpp
 * (dbk_sao_decide_entry, sao_decide_host.h).  Every operand is checked before the context is looked
 * into or the device is touched, in the order the header lists; nothing is enqueued on refusal.  Kernels: sao_decide.hip, sao_pick_os.hip,
 * sao_slice.hip.
 */
#include "deblock_ctx.h"
#include "deblock_host_args.h"
#include "sao_decide_host.h"
#include "sao_decide_launch.h"
#include "sao_pick_os_launch.h"
#include "sao_slice_launch.h"

using namespace dbkh;

static_assert(sizeof(hevcdbk_sao_decision) == 32 && sizeof(DbkSaoDecision) == 32, "hevcdbk_sao_decision is 32 bytes");
static_assert(offsetof(hevcdbk_sao_decision, merge) == offsetof(DbkSaoDecision, merge) && offsetof(hevcdbk_sao_decision, cand) == offsetof(DbkSaoDecision, cand),
              "the kernels' record is the header's");

static_assert(sizeof(hevcdbk_sao_slice_record) == 72 && sizeof(DbkSaoSliceRecord) == 72, "hevcdbk_sao_slice_record is 72 bytes");
static_assert(offsetof(hevcdbk_sao_slice_record, cost_hi) == offsetof(DbkSaoSliceRecord, cost_hi) &&
                  offsetof(hevcdbk_sao_slice_record, flags) == offsetof(DbkSaoSliceRecord, flags),
              "the kernels' slice record is the header's");

/* hevcdbk_sao_decide_device (scale == nullptr: the NEW kernel without scales), hevcdbk_sao_decide_device_os (scale[0], scale[1] =
 * log2_offset_scale_luma, _chroma) and, with so, the two entries that know the slice-level flags: one list of checks, those of the
 * scales and of the flags in the places the header names */
int dbk_sao_decide_entry(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb, const hevcdbk_sao_stats *stats_cr,
                      unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                      unsigned bit_depth_chroma, const unsigned *scale, unsigned lambda_q8_luma, unsigned lambda_q8_chroma, const uint16_t *slice_idx,
                      const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb,
                      hevcdbk_sao_ctb *params_cr, unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision,
                      unsigned decision_stride, size_t decision_frame_stride, const DbkSaoSliceOps *so, void *hip_stream)
{
    const bool chroma = stats_cb != nullptr;
    if (!ctx || !stats_y || !params_y || !decision) return HEVCDBK_ERR_ARG;
    if (chroma != (stats_cr != nullptr)) return HEVCDBK_ERR_ARG;
    if (chroma && (!params_cb || !params_cr)) return HEVCDBK_ERR_ARG;
    if (bit_depth_luma < 8 || bit_depth_luma > 16 || (chroma && (bit_depth_chroma < 8 || bit_depth_chroma > 16))) return HEVCDBK_ERR_ARG;
    if (lambda_q8_luma > (1u << 24) || (chroma && lambda_q8_chroma > (1u << 24))) return HEVCDBK_ERR_ARG;
    auto legal = [](unsigned depth) { return depth > 10 ? depth - 10 : 0u; }; /* the largest scale a stream codes at this depth */
    if (scale && (scale[0] > legal(bit_depth_luma) || (chroma && scale[1] > legal(bit_depth_chroma)))) return HEVCDBK_ERR_ARG;
    if (ctbs_x == 0 || ctbs_y == 0 || ctbs_x > 65535 || ctbs_y > 65535) return HEVCDBK_ERR_DIMENSIONS;
    const bool idx = slice_idx || tile_idx;
    if (stats_stride < ctbs_x || params_stride < ctbs_x || decision_stride < ctbs_x || (idx && idx_stride < ctbs_x)) return HEVCDBK_ERR_ARG;
    if (stats_stride > 0x7fffffffu || params_stride > 0x7fffffffu || decision_stride > 0x7fffffffu || idx_stride > 0x7fffffffu) return HEVCDBK_ERR_ARG;
    if (so && (so->n_slices == 0 || so->n_slices > 65536)) return HEVCDBK_ERR_ARG;
    if (n_frames > 1 && (params_frame_stride < (size_t)params_stride * ctbs_y || decision_frame_stride < (size_t)decision_stride * ctbs_y))
        return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    if (so && n_frames > 1) { /* the flag bytes: shared as an input alone; the slice records likewise an output */
        if (so->flags_frame_stride < so->n_slices && (so->choose || so->flags_frame_stride != 0)) return HEVCDBK_ERR_ARG;
        if (so->choose && so->record && so->record_frame_stride < so->n_slices) return HEVCDBK_ERR_ARG;
    }
    if (n_frames > 65535) return HEVCDBK_ERR_ARG;
    if ((uintptr_t)stats_y % 4 != 0 || (uintptr_t)stats_cb % 4 != 0 || (uintptr_t)stats_cr % 4 != 0 || (uintptr_t)decision % 8 != 0 ||
        (uintptr_t)slice_idx % 2 != 0 || (uintptr_t)tile_idx % 2 != 0)
        return HEVCDBK_ERR_ARG;
    if (so && so->choose) {
        if (!so->flags_out || !so->workspace || (uintptr_t)so->workspace % 16 != 0 || (uintptr_t)so->record % 8 != 0) return HEVCDBK_ERR_ARG;
        if (so->workspace_bytes < hevcdbk_sao_slice_flags_workspace(ctbs_x, ctbs_y, n_frames, so->n_slices)) return HEVCDBK_ERR_ARG;
    }
    if (n_frames > 0) { /* from an array's first entry to its last: no output's extent meets another's, or that of the statistics */
        struct Extent {
            uintptr_t lo, hi;
        };
        auto extent = [&](const void *p, unsigned stride, size_t frame_stride, size_t entry) {
            const unsigned long long n = (unsigned long long)(n_frames - 1) * frame_stride + (unsigned long long)(ctbs_y - 1) * stride + ctbs_x;
            return Extent{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(n * entry)};
        };
        auto run = [&](const void *p, size_t n, size_t frame_stride, size_t entry) { /* n entries per frame */
            return Extent{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(((unsigned long long)(n_frames - 1) * frame_stride + n) * entry)};
        };
        Extent e[11];
        int n_out = 0, n_all;
        e[n_out++] = extent(params_y, params_stride, params_frame_stride, sizeof(hevcdbk_sao_ctb));
        e[n_out++] = extent(decision, decision_stride, decision_frame_stride, sizeof(hevcdbk_sao_decision));
        if (chroma) {
            e[n_out++] = extent(params_cb, params_stride, params_frame_stride, sizeof(hevcdbk_sao_ctb));
            e[n_out++] = extent(params_cr, params_stride, params_frame_stride, sizeof(hevcdbk_sao_ctb));
        }
        if (so && so->choose) {
            e[n_out++] = run(so->flags_out, so->n_slices, so->flags_frame_stride, 1);
            e[n_out++] = run(so->workspace, so->workspace_bytes, 0, 1);
            if (so->record) e[n_out++] = run(so->record, so->n_slices, so->record_frame_stride, sizeof(hevcdbk_sao_slice_record));
        }
        n_all = n_out;
        if (so && !so->choose) e[n_all++] = run(so->flags_in, so->n_slices, so->flags_frame_stride, 1);
        e[n_all++] = extent(stats_y, stats_stride, stats_frame_stride, sizeof(hevcdbk_sao_stats));
        if (chroma) {
            e[n_all++] = extent(stats_cb, stats_stride, stats_frame_stride, sizeof(hevcdbk_sao_stats));
            e[n_all++] = extent(stats_cr, stats_stride, stats_frame_stride, sizeof(hevcdbk_sao_stats));
        }
        for (int i = 0; i < n_out; i++)
            for (int k = i + 1; k < n_all; k++)
                if (e[i].lo < e[k].hi && e[k].lo < e[i].hi) return HEVCDBK_ERR_ARG;
    }
    DbkSaoDecideArgs a = {};
    a.stats_y = reinterpret_cast<const int32_t *>(stats_y);
    a.stats_cb = reinterpret_cast<const int32_t *>(stats_cb);
    a.stats_cr = reinterpret_cast<const int32_t *>(stats_cr);
    a.stats_stride = (int)stats_stride; a.stats_frame_stride = (long long)stats_frame_stride;
    a.ctbs_x = (int)ctbs_x; a.ctbs_y = (int)ctbs_y; a.n_frames = (int)n_frames;
    a.max_offset_luma = (1 << ((bit_depth_luma < 10 ? bit_depth_luma : 10) - 5)) - 1;
    a.lambda_luma = (long long)lambda_q8_luma;
    if (chroma) {
        a.max_offset_chroma = (1 << ((bit_depth_chroma < 10 ? bit_depth_chroma : 10) - 5)) - 1;
        a.lambda_chroma = (long long)lambda_q8_chroma;
        a.params_cb = reinterpret_cast<DbkSaoCtb *>(params_cb);
        a.params_cr = reinterpret_cast<DbkSaoCtb *>(params_cr);
    }
    a.slice_idx = slice_idx; a.tile_idx = tile_idx;
    a.idx_stride = (int)idx_stride; a.idx_frame_stride = (long long)idx_frame_stride;
    a.params_y = reinterpret_cast<DbkSaoCtb *>(params_y);
    a.params_stride = (int)params_stride; a.params_frame_stride = (long long)params_frame_stride;
    a.decision = reinterpret_cast<DbkSaoDecision *>(decision);
    a.decision_stride = (int)decision_stride; a.decision_frame_stride = (long long)decision_frame_stride;
    if (scale && (scale[0] > 2 || (chroma && scale[1] > 2))) return HEVCDBK_ERR_UNSUPPORTED; /* 31 << 3 leaves int8_t */
    if (so && so->choose && so->n_slices > (unsigned)saoslice::kMaxSlices) return HEVCDBK_ERR_UNSUPPORTED; /* a frame's sums live in LDS */
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (so) {
        DbkSaoSliceArgs sa = {};
        sa.o = DbkSaoDecideOsArgs{a, (int)scale[0], chroma ? (int)scale[1] : 0};
        sa.n_slices = (int)so->n_slices;
        sa.flags_frame_stride = (long long)so->flags_frame_stride;
        if (!so->choose) {
            sa.flags_in = so->flags_in;
            return hip_ok(ctx, dbk_launch_sao_decide_sf(sa, s), "SAO decide launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
        }
        sa.flags_out = so->flags_out;
        sa.record = reinterpret_cast<DbkSaoSliceRecord *>(so->record);
        sa.record_frame_stride = (long long)so->record_frame_stride;
        sa.ws_decision = static_cast<DbkSaoDecision *>(so->workspace); /* [frame][pair][ctb] records, then the parameter grids */
        sa.ws_params = reinterpret_cast<DbkSaoCtb *>(sa.ws_decision + 3ull * n_frames * ctbs_x * ctbs_y);
        return hip_ok(ctx, dbk_launch_sao_slice_flags(sa, s), "SAO slice flags launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    }
    if (!scale) return hip_ok(ctx, dbk_launch_sao_decide(a, s), "SAO decide launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    const DbkSaoDecideOsArgs o = {a, (int)scale[0], chroma ? (int)scale[1] : 0};
    return hip_ok(ctx, dbk_launch_sao_decide_os(o, s), "SAO decide launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

extern "C" {

int hevcdbk_sao_decide_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                              const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x,
                              unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma, unsigned bit_depth_chroma, unsigned lambda_q8_luma,
                              unsigned lambda_q8_chroma, const uint16_t *slice_idx, const uint16_t *tile_idx, unsigned idx_stride,
                              size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr,
                              unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                              size_t decision_frame_stride, void *hip_stream)
{
    return dbk_sao_decide_entry(ctx, stats_y, stats_cb, stats_cr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth_luma, bit_depth_chroma,
                      nullptr, lambda_q8_luma, lambda_q8_chroma, slice_idx, tile_idx, idx_stride, idx_frame_stride, params_y, params_cb, params_cr,
                      params_stride, params_frame_stride, decision, decision_stride, decision_frame_stride, nullptr, hip_stream);
}

int hevcdbk_sao_decide_device_os(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                 const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x,
                                 unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma, unsigned bit_depth_chroma,
                                 unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma, unsigned lambda_q8_luma,
                                 unsigned lambda_q8_chroma, const uint16_t *slice_idx, const uint16_t *tile_idx, unsigned idx_stride,
                                 size_t idx_frame_stride, hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr,
                                 unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                 size_t decision_frame_stride, void *hip_stream)
{
    const unsigned scale[2] = {log2_offset_scale_luma, log2_offset_scale_chroma};
    return dbk_sao_decide_entry(ctx, stats_y, stats_cb, stats_cr, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth_luma, bit_depth_chroma,
                      scale, lambda_q8_luma, lambda_q8_chroma, slice_idx, tile_idx, idx_stride, idx_frame_stride, params_y, params_cb, params_cr,
                      params_stride, params_frame_stride, decision, decision_stride, decision_frame_stride, nullptr, hip_stream);
}

} /* extern "C" */
