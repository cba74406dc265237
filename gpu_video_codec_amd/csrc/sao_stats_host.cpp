/*
 * sao_stats_host.cpp -- C-ABI entries of SAO parameter estimation: hevcdbk_sao_stats_device (per-CTB statistics of a deblocked plane
 * against the original), hevcdbk_sao_stats_device_sp (the same of a plane of interleaved Cb / Cr pairs, one array per component) and
 * hevcdbk_sao_pick_device / _os (hevcdbk_sao_ctb from those statistics, the second with log2_sao_offset_scale).  Every operand is checked before the context is looked into or the
 * device is touched; nothing is enqueued on refusal.  Kernels: sao_stats.hip, sao_stats_sp.hip, sao_pick_os.hip.
 */
#include "deblock_ctx.h"
#include "deblock_host_args.h"
#include "sao_pick_os_launch.h"
#include "sao_stats_launch.h"
#include "sao_stats_sp_launch.h"

using namespace dbkh;

static_assert(sizeof(hevcdbk_sao_stats) == 384 && sizeof(hevcdbk_sao_stats) == saostats::kBins * sizeof(int32_t), "hevcdbk_sao_stats is 96 int32");

extern "C" {

int hevcdbk_sao_stats_device(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch, size_t org_frame_stride,
                             unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                             const hevcdbk_sao_borders *borders, hevcdbk_sao_stats *stats, unsigned stats_stride, size_t stats_frame_stride,
                             void *hip_stream)
{
    if (!ctx || !rec || !rec->src || !org || !stats) return HEVCDBK_ERR_ARG;
    if (bad_depth(rec->bit_depth, rec->sample_bytes)) return HEVCDBK_ERR_ARG;
    if (g4_kind(rec->plane_w, rec->plane_h) < 0) return HEVCDBK_ERR_DIMENSIONS;
    if (ctb_log2_w < 3 || ctb_log2_w > 6 || (ctb_log2_h != ctb_log2_w && ctb_log2_h != ctb_log2_w + 1) || ctb_log2_h > 6) return HEVCDBK_ERR_ARG;
    const unsigned sb = rec->sample_bytes;
    const unsigned ctbs_x = (rec->plane_w + (1u << ctb_log2_w) - 1) >> ctb_log2_w, ctbs_y = (rec->plane_h + (1u << ctb_log2_h) - 1) >> ctb_log2_h;
    if (rec->pitch < (size_t)rec->plane_w * sb || org_pitch < (size_t)rec->plane_w * sb || rec->n_frames > 65535 || rec->plane_h > 65535)
        return HEVCDBK_ERR_ARG;
    if (keep && keep_stride < (rec->plane_w + 7) / 8) return HEVCDBK_ERR_ARG;
    if (borders && (!borders->nox || borders->stride < ctbs_x)) return HEVCDBK_ERR_ARG;
    if (stats_stride < ctbs_x || stats_stride > 0x7fffffffu || (uintptr_t)stats % 4 != 0) return HEVCDBK_ERR_ARG;
    if (rec->n_frames > 1 && stats_frame_stride < (size_t)stats_stride * ctbs_y) return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    /* samples at addresses that are no multiple of their size */
    if (rec->pitch % sb != 0 || rec->frame_stride % sb != 0 || (uintptr_t)rec->src % sb != 0 || org_pitch % sb != 0 || org_frame_stride % sb != 0 ||
        (uintptr_t)org % sb != 0)
        return HEVCDBK_ERR_UNSUPPORTED;
    DbkSaoStatsArgs a = {};
    a.rec = (const uint8_t *)rec->src;
    a.org = (const uint8_t *)org;
    a.rec_pitch = (long long)rec->pitch; a.rec_frame_stride = (long long)rec->frame_stride;
    a.org_pitch = (long long)org_pitch; a.org_frame_stride = (long long)org_frame_stride;
    a.plane_w = (int)rec->plane_w; a.plane_h = (int)rec->plane_h; a.n_frames = (int)rec->n_frames;
    a.band_shift = (int)rec->bit_depth - 5;
    a.lw = (int)ctb_log2_w; a.lh = (int)ctb_log2_h;
    a.keep = keep; a.keep_stride = (int)keep_stride; a.keep_frame_stride = (long long)keep_frame_stride;
    if (borders) {
        a.nox = borders->nox; a.nox_stride = (int)borders->stride; a.nox_frame_stride = (long long)borders->frame_stride;
    }
    a.stats = reinterpret_cast<int32_t *>(stats);
    a.stats_stride = (int)stats_stride; a.stats_frame_stride = (long long)stats_frame_stride;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    return hip_ok(ctx, dbk_launch_sao_stats(a, (int)sb, s), "SAO statistics launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* a plane of interleaved Cb / Cr pairs: the checks of hevcdbk_sao_stats_device in its order, with what a pair plane adds in the place
 * of what it replaces -- is_chroma beside the depth, a pitch of two samples per pair, two outputs that must not overlap */
int hevcdbk_sao_stats_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch, size_t org_frame_stride,
                                unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                                const hevcdbk_sao_borders *borders, hevcdbk_sao_stats *stats_cb, hevcdbk_sao_stats *stats_cr,
                                unsigned stats_stride, size_t stats_frame_stride, void *hip_stream)
{
    if (!ctx || !rec || !rec->src || !org || !stats_cb || !stats_cr) return HEVCDBK_ERR_ARG;
    if (bad_depth(rec->bit_depth, rec->sample_bytes) || !rec->is_chroma) return HEVCDBK_ERR_ARG;
    if (g4_kind(rec->plane_w, rec->plane_h) < 0) return HEVCDBK_ERR_DIMENSIONS;
    if (ctb_log2 < 3 || ctb_log2 > 5) return HEVCDBK_ERR_ARG;
    const unsigned sb = rec->sample_bytes;
    const unsigned ctbs_x = (rec->plane_w + (1u << ctb_log2) - 1) >> ctb_log2, ctbs_y = (rec->plane_h + (1u << ctb_log2) - 1) >> ctb_log2;
    if (rec->pitch < 2 * (size_t)rec->plane_w * sb || org_pitch < 2 * (size_t)rec->plane_w * sb || rec->n_frames > 65535 || rec->plane_h > 65535)
        return HEVCDBK_ERR_ARG;
    if (keep && keep_stride < (rec->plane_w + 7) / 8) return HEVCDBK_ERR_ARG;
    if (borders && (!borders->nox || borders->stride < ctbs_x)) return HEVCDBK_ERR_ARG;
    if (stats_stride < ctbs_x || stats_stride > 0x7fffffffu || (uintptr_t)stats_cb % 4 != 0 || (uintptr_t)stats_cr % 4 != 0) return HEVCDBK_ERR_ARG;
    if (rec->n_frames > 1 && stats_frame_stride < (size_t)stats_stride * ctbs_y) return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    if (rec->n_frames > 0) { /* from an array's first entry to its last: the two extents apart */
        const unsigned long long span = (((unsigned long long)(rec->n_frames - 1) * stats_frame_stride + (unsigned long long)(ctbs_y - 1) * stats_stride + ctbs_x)) *
                                        sizeof(hevcdbk_sao_stats);
        const uintptr_t cb = (uintptr_t)stats_cb, cr = (uintptr_t)stats_cr;
        if (cb < cr ? cr - cb < span : cb - cr < span) return HEVCDBK_ERR_ARG;
    }
    /* samples at addresses that are no multiple of their size */
    if (rec->pitch % sb != 0 || rec->frame_stride % sb != 0 || (uintptr_t)rec->src % sb != 0 || org_pitch % sb != 0 || org_frame_stride % sb != 0 ||
        (uintptr_t)org % sb != 0)
        return HEVCDBK_ERR_UNSUPPORTED;
    DbkSaoStatsSpArgs sp = {};
    DbkSaoStatsArgs &a = sp.p;
    a.rec = (const uint8_t *)rec->src;
    a.org = (const uint8_t *)org;
    a.rec_pitch = (long long)rec->pitch; a.rec_frame_stride = (long long)rec->frame_stride;
    a.org_pitch = (long long)org_pitch; a.org_frame_stride = (long long)org_frame_stride;
    a.plane_w = (int)rec->plane_w; a.plane_h = (int)rec->plane_h; a.n_frames = (int)rec->n_frames;
    a.band_shift = (int)rec->bit_depth - 5;
    a.lw = a.lh = (int)ctb_log2;
    a.keep = keep; a.keep_stride = (int)keep_stride; a.keep_frame_stride = (long long)keep_frame_stride;
    if (borders) {
        a.nox = borders->nox; a.nox_stride = (int)borders->stride; a.nox_frame_stride = (long long)borders->frame_stride;
    }
    a.stats = reinterpret_cast<int32_t *>(stats_cb);
    sp.stats_cr = reinterpret_cast<int32_t *>(stats_cr);
    a.stats_stride = (int)stats_stride; a.stats_frame_stride = (long long)stats_frame_stride;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    return hip_ok(ctx, dbk_launch_sao_stats_sp(sp, (int)sb, s), "SAO statistics launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* hevcdbk_sao_pick_device (scale == nullptr: the kernel without a scale) and hevcdbk_sao_pick_device_os (*scale = log2_offset_scale):
 * one list of checks, the two of the scale in the places the header names */
static int sao_pick(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_a, const hevcdbk_sao_stats *stats_b, unsigned stats_stride,
                    size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth, const unsigned *scale,
                    unsigned lambda_q8, hevcdbk_sao_ctb *params_a, hevcdbk_sao_ctb *params_b, unsigned params_stride, size_t params_frame_stride,
                    int64_t *delta_d, void *hip_stream)
{
    if (!ctx || !stats_a || !params_a || (stats_b != nullptr) != (params_b != nullptr)) return HEVCDBK_ERR_ARG;
    if (bit_depth < 8 || bit_depth > 16 || lambda_q8 > (1u << 24)) return HEVCDBK_ERR_ARG;
    if (scale && *scale > (bit_depth > 10 ? bit_depth - 10 : 0u)) return HEVCDBK_ERR_ARG; /* no stream codes it */
    if (ctbs_x == 0 || ctbs_y == 0 || ctbs_x > 0x7fffffffu || ctbs_y > 65535 || n_frames > 65535) return HEVCDBK_ERR_DIMENSIONS;
    if (stats_stride < ctbs_x || params_stride < ctbs_x || stats_stride > 0x7fffffffu || params_stride > 0x7fffffffu) return HEVCDBK_ERR_ARG;
    if ((uintptr_t)stats_a % 4 != 0 || (uintptr_t)stats_b % 4 != 0 || (uintptr_t)delta_d % 8 != 0) return HEVCDBK_ERR_ARG;
    if (n_frames > 1 && params_frame_stride < (size_t)params_stride * ctbs_y) return HEVCDBK_ERR_ARG; /* an output cannot be shared */
    DbkSaoPickArgs a = {};
    a.stats_a = reinterpret_cast<const int32_t *>(stats_a);
    a.stats_b = reinterpret_cast<const int32_t *>(stats_b);
    a.stats_stride = (int)stats_stride; a.stats_frame_stride = (long long)stats_frame_stride;
    a.ctbs_x = (int)ctbs_x; a.ctbs_y = (int)ctbs_y; a.n_frames = (int)n_frames;
    a.max_offset = (1 << ((bit_depth < 10 ? bit_depth : 10) - 5)) - 1;
    a.lambda = (long long)lambda_q8;
    a.params_a = reinterpret_cast<DbkSaoCtb *>(params_a);
    a.params_b = reinterpret_cast<DbkSaoCtb *>(params_b);
    a.params_stride = (int)params_stride; a.params_frame_stride = (long long)params_frame_stride;
    a.delta_d = reinterpret_cast<long long *>(delta_d);
    if (scale && *scale > 2) return HEVCDBK_ERR_UNSUPPORTED; /* 31 << 3 leaves int8_t */
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (!scale) return hip_ok(ctx, dbk_launch_sao_pick(a, s), "SAO pick launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    const DbkSaoPickOsArgs o = {a, (int)*scale};
    return hip_ok(ctx, dbk_launch_sao_pick_os(o, s), "SAO pick launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

int hevcdbk_sao_pick_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_a, const hevcdbk_sao_stats *stats_b, unsigned stats_stride,
                            size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth,
                            unsigned lambda_q8, hevcdbk_sao_ctb *params_a, hevcdbk_sao_ctb *params_b, unsigned params_stride,
                            size_t params_frame_stride, int64_t *delta_d, void *hip_stream)
{
    return sao_pick(ctx, stats_a, stats_b, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth, nullptr, lambda_q8, params_a,
                    params_b, params_stride, params_frame_stride, delta_d, hip_stream);
}

int hevcdbk_sao_pick_device_os(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_a, const hevcdbk_sao_stats *stats_b, unsigned stats_stride,
                               size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth,
                               unsigned log2_offset_scale, unsigned lambda_q8, hevcdbk_sao_ctb *params_a, hevcdbk_sao_ctb *params_b,
                               unsigned params_stride, size_t params_frame_stride, int64_t *delta_d, void *hip_stream)
{
    return sao_pick(ctx, stats_a, stats_b, stats_stride, stats_frame_stride, ctbs_x, ctbs_y, n_frames, bit_depth, &log2_offset_scale, lambda_q8,
                    params_a, params_b, params_stride, params_frame_stride, delta_d, hip_stream);
}

} /* extern "C" */
