/*
 * sse_host.cpp -- C-ABI entries of measured distortion: hevcdbk_sse_device (the sum of squared errors of a plane against the original,
 * per CTB), hevcdbk_sse_device_sp (the same of a plane of interleaved Cb / Cr pairs, one array per component) and
 * hevcdbk_sse_totals_device (those sums per slice and per frame).  Every operand is checked before the context is looked into or the
 * device is touched; nothing is enqueued on refusal.  Kernels: sse.hip.
 */
#include "deblock_ctx.h"
#include "deblock_host_args.h"
#include "sse_launch.h"

using namespace dbkh;

namespace {

/* two runs of memory, `na` bytes at a and `nb` bytes at b, share a byte */
bool meet(const void *a, unsigned long long na, const void *b, unsigned long long nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && (x < y ? y - x < na : x - y < nb);
}

/* hevcdbk_sse_device (sse_cr == nullptr, pairs == false) and hevcdbk_sse_device_sp: one list of checks, in the order of
 * hevcdbk_sao_stats_device / _sp, with what a pair plane replaces in its place */
int sse_entry(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch, size_t org_frame_stride, unsigned lw,
              unsigned lh, bool pairs, uint64_t *sse, uint64_t *sse_cr, unsigned sse_stride, size_t sse_frame_stride, void *hip_stream)
{
    if (!ctx || !rec || !rec->src || !org || !sse || (pairs && !sse_cr)) return HEVCDBK_ERR_ARG;
    if (bad_depth(rec->bit_depth, rec->sample_bytes) || (pairs && !rec->is_chroma)) return HEVCDBK_ERR_ARG;
    if (g4_kind(rec->plane_w, rec->plane_h) < 0) return HEVCDBK_ERR_DIMENSIONS;
    if (pairs ? (lw < 3 || lw > 5) : (lw < 3 || lw > 6 || (lh != lw && lh != lw + 1) || lh > 6)) return HEVCDBK_ERR_ARG;
    const unsigned sb = rec->sample_bytes;
    const unsigned ctbs_x = (rec->plane_w + (1u << lw) - 1) >> lw, ctbs_y = (rec->plane_h + (1u << lh) - 1) >> lh;
    const size_t row = (pairs ? 2 : 1) * (size_t)rec->plane_w * sb;
    if (rec->pitch < row || org_pitch < row || rec->n_frames > 65535 || rec->plane_h > 65535) return HEVCDBK_ERR_ARG;
    if (sse_stride < ctbs_x || sse_stride > 0x7fffffffu || (uintptr_t)sse % 8 != 0 || (uintptr_t)sse_cr % 8 != 0) return HEVCDBK_ERR_ARG;
    if (rec->n_frames > 1 && sse_frame_stride < (size_t)sse_stride * ctbs_y) return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    if (pairs && rec->n_frames > 0) { /* from an array's first entry to its last: the two extents apart */
        const unsigned long long span =
            ((unsigned long long)(rec->n_frames - 1) * sse_frame_stride + (unsigned long long)(ctbs_y - 1) * sse_stride + ctbs_x) * sizeof(uint64_t);
        if (meet(sse, span, sse_cr, span)) return HEVCDBK_ERR_ARG;
    }
    /* samples at addresses that are no multiple of their size */
    if (rec->pitch % sb != 0 || rec->frame_stride % sb != 0 || (uintptr_t)rec->src % sb != 0 || org_pitch % sb != 0 || org_frame_stride % sb != 0 ||
        (uintptr_t)org % sb != 0)
        return HEVCDBK_ERR_UNSUPPORTED;
    DbkSseArgs a = {};
    a.rec = (const uint8_t *)rec->src;
    a.org = (const uint8_t *)org;
    a.rec_pitch = (long long)rec->pitch; a.rec_frame_stride = (long long)rec->frame_stride;
    a.org_pitch = (long long)org_pitch; a.org_frame_stride = (long long)org_frame_stride;
    a.plane_w = (int)rec->plane_w; a.plane_h = (int)rec->plane_h; a.n_frames = (int)rec->n_frames;
    a.lw = (int)lw; a.lh = (int)lh;
    a.wide_acc = rec->bit_depth > (unsigned)sse::kAcc32MaxDepth;
    a.sse = reinterpret_cast<unsigned long long *>(sse);
    a.sse_odd = reinterpret_cast<unsigned long long *>(sse_cr);
    a.sse_stride = (int)sse_stride; a.sse_frame_stride = (long long)sse_frame_stride;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const hipError_t e = pairs ? dbk_launch_sse_sp(a, (int)sb, s) : dbk_launch_sse(a, (int)sb, s);
    return hip_ok(ctx, e, "SSE launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

} /* namespace */

extern "C" {

int hevcdbk_sse_device(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch, size_t org_frame_stride,
                       unsigned ctb_log2_w, unsigned ctb_log2_h, uint64_t *sse, unsigned sse_stride, size_t sse_frame_stride, void *hip_stream)
{
    return sse_entry(ctx, rec, org, org_pitch, org_frame_stride, ctb_log2_w, ctb_log2_h, false, sse, nullptr, sse_stride, sse_frame_stride, hip_stream);
}

int hevcdbk_sse_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch, size_t org_frame_stride,
                          unsigned ctb_log2, uint64_t *sse_cb, uint64_t *sse_cr, unsigned sse_stride, size_t sse_frame_stride, void *hip_stream)
{
    return sse_entry(ctx, rec, org, org_pitch, org_frame_stride, ctb_log2, ctb_log2, true, sse_cb, sse_cr, sse_stride, sse_frame_stride, hip_stream);
}

int hevcdbk_sse_totals_device(hevcdbk_context *ctx, const uint64_t *sse, unsigned sse_stride, size_t sse_frame_stride, unsigned ctbs_x,
                              unsigned ctbs_y, unsigned n_frames, const uint16_t *slice_idx, unsigned idx_stride, size_t idx_frame_stride,
                              unsigned n_slices, uint64_t *slice_total, size_t slice_total_frame_stride, uint64_t *frame_total, void *hip_stream)
{
    if (!ctx || !sse || (!slice_total && !frame_total)) return HEVCDBK_ERR_ARG;
    if (ctbs_x == 0 || ctbs_y == 0 || ctbs_x > 65535 || ctbs_y > 65535) return HEVCDBK_ERR_DIMENSIONS;
    if (sse_stride < ctbs_x || sse_stride > 0x7fffffffu || (slice_idx && (idx_stride < ctbs_x || idx_stride > 0x7fffffffu))) return HEVCDBK_ERR_ARG;
    if (n_slices == 0 || n_slices > 65536) return HEVCDBK_ERR_ARG;
    if (n_frames > 65535) return HEVCDBK_ERR_ARG;
    if (n_frames > 1 && slice_total && slice_total_frame_stride < n_slices) return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    if ((uintptr_t)sse % 8 != 0 || (uintptr_t)slice_total % 8 != 0 || (uintptr_t)frame_total % 8 != 0 || (uintptr_t)slice_idx % 2 != 0)
        return HEVCDBK_ERR_ARG;
    if (n_frames > 0) {
        const unsigned long long last = n_frames - 1;
        const unsigned long long in = (last * sse_frame_stride + (unsigned long long)(ctbs_y - 1) * sse_stride + ctbs_x) * sizeof(uint64_t);
        const unsigned long long st = (last * slice_total_frame_stride + n_slices) * sizeof(uint64_t), ft = (last + 1) * sizeof(uint64_t);
        if (meet(slice_total, st, frame_total, ft) || meet(slice_total, st, sse, in) || meet(frame_total, ft, sse, in)) return HEVCDBK_ERR_ARG;
    }
    if (n_slices > (unsigned)sse::kMaxSlices) return HEVCDBK_ERR_UNSUPPORTED; /* the totals of a frame live in LDS */
    DbkSseTotalsArgs a = {};
    a.sse = reinterpret_cast<const unsigned long long *>(sse);
    a.sse_stride = (int)sse_stride; a.sse_frame_stride = (long long)sse_frame_stride;
    a.ctbs_x = (int)ctbs_x; a.ctbs_y = (int)ctbs_y; a.n_frames = (int)n_frames;
    a.slice_idx = slice_idx; a.idx_stride = (int)idx_stride; a.idx_frame_stride = (long long)idx_frame_stride;
    a.n_slices = (int)n_slices;
    a.slice_total = reinterpret_cast<unsigned long long *>(slice_total);
    a.slice_total_frame_stride = (long long)slice_total_frame_stride;
    a.frame_total = reinterpret_cast<unsigned long long *>(frame_total);
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    return hip_ok(ctx, dbk_launch_sse_totals(a, s), "SSE totals launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

} /* extern "C" */
