/*
 * deblock_host_args.h -- PRIVATE to the library: what the C-ABI entries of the spec-exact mode and of SAO share when they check their
 * operands and fill the launch arguments (deblock_host_h265.cpp; deblock_host_sp.cpp: the fused entries of a semi-planar picture), and
 * the two-launch form of deblocking + SAO through the context's scratch plane.  Nothing here is exported.
 */
#pragma once
#include <cstring>

#include "deblock_ctx.h"

namespace dbkh {

/* SubWidthC / SubHeightC of chroma_format_idc 1..3 (H.265 Table 6-1) */
inline unsigned sub_w(int cf) { return cf == HEVCDBK_CHROMA_444 ? 1u : 2u; }
inline unsigned sub_h(int cf) { return cf == HEVCDBK_CHROMA_420 ? 2u : 1u; }

/* a plane size: 0 = multiples of 8 (what every entry takes), 1 = multiples of 4 and at least 8 with one of them not a multiple of 8
 * (a "g4 plane": the _g4 entries), -1 = anything else */
inline int g4_kind(unsigned w, unsigned h)
{
    if (w < 8 || h < 8 || w % 4 != 0 || h % 4 != 0) return -1;
    return (w % 8 != 0 || h % 8 != 0) ? 1 : 0;
}

/* planes_to_args for the _g4 entries: a g4 plane passes every check planes_to_args makes of a plane -- on its size rounded down to
 * multiples of 8, which is still a plane -- and then gets its own geometry: the block counts and the vertical array's stride are
 * plane / 8 + 1 with floor division, as for every plane */
inline int planes_to_args_g4(const hevcdbk_device_planes *p, unsigned qp, DbkArgs &a)
{
    if (!p || g4_kind(p->plane_w, p->plane_h) != 1) return planes_to_args(p, qp, nullptr, a);
    hevcdbk_device_planes q = *p;
    q.plane_w = p->plane_w & ~7u;
    q.plane_h = p->plane_h & ~7u;
    if (int rc = planes_to_args(&q, qp, nullptr, a)) return rc;
    if (p->pitch < (size_t)p->plane_w * p->sample_bytes) return HEVCDBK_ERR_ARG;
    a.plane_w = (int)p->plane_w;
    a.plane_h = (int)p->plane_h;
    a.nbx = a.vstride = (int)(p->plane_w / 8 + 1);
    a.nby = (int)(p->plane_h / 8 + 1);
    return HEVCDBK_OK;
}

inline int h265_args(const hevcdbk_device_planes *planes, int c_idx, unsigned qp, const hevcdbk_h265_params *prm, DbkH265Args &h, bool g4 = false)
{
    if (!planes || c_idx < 0 || c_idx > 2 || (c_idx != 0) != (planes->is_chroma != 0)) return HEVCDBK_ERR_ARG;
    const hevcdbk_h265_params zero = {0, 0, 0, 0};
    if (!prm) prm = &zero;
    if (prm->tc_offset_div2 < -6 || prm->tc_offset_div2 > 6 || prm->beta_offset_div2 < -6 || prm->beta_offset_div2 > 6 ||
        prm->cb_qp_offset < -12 || prm->cb_qp_offset > 12 || prm->cr_qp_offset < -12 || prm->cr_qp_offset > 12)
        return HEVCDBK_ERR_ARG;
    if (planes->qp_map && (planes->ctu_log2 < 3 || planes->ctu_log2 > 8)) return HEVCDBK_ERR_ARG;
    if (int rc = g4 ? planes_to_args_g4(planes, qp, h.base) : planes_to_args(planes, qp, nullptr, h.base)) return rc;
    if (g4 && c_idx == 0 && g4_kind(planes->plane_w, planes->plane_h) != 0) return HEVCDBK_ERR_DIMENSIONS; /* HEVC has no such luma plane */
    h.base.hstride = (int)(planes->plane_w / 4);
    h.base.n_vert = (int)hevcdbk_h265_num_vert_bs(planes->plane_w, planes->plane_h);
    h.base.n_hor = (int)hevcdbk_h265_num_hor_bs(planes->plane_w, planes->plane_h);
    h.qp = (int)(qp > 51 ? 51 : qp);
    h.tc_off = prm->tc_offset_div2 * 2;
    h.beta_off = prm->beta_offset_div2 * 2;
    h.c_qp_offset = c_idx == 1 ? prm->cb_qp_offset : (c_idx == 2 ? prm->cr_qp_offset : 0);
    return HEVCDBK_OK;
}

/* h265_args with the picture's chroma format: 4:0:0 has no chroma plane */
inline int h265_args_cf(const hevcdbk_device_planes *planes, int c_idx, int cf, unsigned qp, const hevcdbk_h265_params *prm, DbkH265Args &h,
                        bool g4 = false)
{
    if (cf < HEVCDBK_CHROMA_400 || cf > HEVCDBK_CHROMA_444) return HEVCDBK_ERR_ARG;
    if (cf == HEVCDBK_CHROMA_400 && (c_idx != 0 || (planes && planes->is_chroma))) return HEVCDBK_ERR_ARG;
    return h265_args(planes, c_idx, qp, prm, h, g4);
}

/* "no per-slice offsets" for the _g4 / _sp kernels: an array of no bytes, every pair of which reads (0, 0) */
static const DbkSlOffs kNoSlOffs = {nullptr, 0, 0, 4, 0u};

/* validates the operand against the LUMA picture of plane p (c_idx 0: the plane itself; else scaled by the format) and fills sl */
inline int sl_args(const hevcdbk_h265_slice_offsets *so, const hevcdbk_device_planes *p, int c_idx, int cf, DbkSlOffs &sl)
{
    if (!so->offs || (uintptr_t)so->offs % 2 != 0 || so->frame_stride % 2 != 0 || so->ctb_log2 < 4 || so->ctb_log2 > 6) return HEVCDBK_ERR_ARG;
    const unsigned long long lw = (unsigned long long)p->plane_w * (c_idx ? sub_w(cf) : 1u), lh = (unsigned long long)p->plane_h * (c_idx ? sub_h(cf) : 1u);
    const unsigned long long cols = (lw + (1u << so->ctb_log2) - 1) >> so->ctb_log2, rows = (lh + (1u << so->ctb_log2) - 1) >> so->ctb_log2;
    if (so->stride < cols || so->stride >= (1u << 23)) return HEVCDBK_ERR_ARG; /* 2 * stride is a 24-bit multiplicand of the kernels */
    const unsigned long long bytes = 2ull * so->stride * rows;
    if (bytes > 0x7fffffffull || rows >= (1u << 24)) return HEVCDBK_ERR_ARG;
    sl.offs = so->offs;
    sl.stride = (int)so->stride;
    sl.frame_stride = (long long)so->frame_stride;
    sl.ctb_log2 = (int)so->ctb_log2;
    sl.n_bytes = (uint32_t)bytes;
    return HEVCDBK_OK;
}

/* the operand of a _g4 launch: the caller's array -- then the call's own pair, which the kernels add, is zero (8.7.2.5.3: the pair is
 * the slice's) -- or none */
inline int sl_args_g4(const hevcdbk_h265_slice_offsets *so, const hevcdbk_device_planes *p, int c_idx, int cf, DbkH265Args &h, DbkSlOffs &sl)
{
    if (!so) {
        sl = kNoSlOffs;
        return HEVCDBK_OK;
    }
    if (int rc = sl_args(so, p, c_idx, cf, sl)) return rc;
    h.tc_off = h.beta_off = 0;
    return HEVCDBK_OK;
}

/* validates the SAO operands of `p` and fills `a` (src / dst as in `p`) */
/* g4 (the _g4 entries): sizes that are multiples of 4 and at least 8; the keep map by ceiling, its last byte of a row / column
 * speaking for 4 samples */
inline int sao_args(const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride,
                    unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, DbkSaoArgs &a, bool g4 = false)
{
    if (!p || !p->src || !p->dst || p->src == p->dst || !params) return HEVCDBK_ERR_ARG;
    if (bad_depth(p->bit_depth, p->sample_bytes)) return HEVCDBK_ERR_ARG;
    if (g4 ? g4_kind(p->plane_w, p->plane_h) < 0 : (p->plane_w == 0 || p->plane_h == 0 || p->plane_w % 8 != 0 || p->plane_h % 8 != 0))
        return HEVCDBK_ERR_DIMENSIONS;
    if (ctb_log2 < 3 || ctb_log2 > 6) return HEVCDBK_ERR_ARG;
    if (params_stride < ((p->plane_w + (1u << ctb_log2) - 1) >> ctb_log2)) return HEVCDBK_ERR_ARG;
    if (keep && keep_stride < (p->plane_w + 7) / 8) return HEVCDBK_ERR_ARG;
    const size_t align = 4 * p->sample_bytes;
    if (p->pitch % align != 0 || p->frame_stride % align != 0 || (uintptr_t)p->src % align != 0 || (uintptr_t)p->dst % align != 0)
        return HEVCDBK_ERR_UNSUPPORTED;
    if (p->pitch < (size_t)p->plane_w * p->sample_bytes || p->n_frames > 65535 || p->plane_h > 65535) return HEVCDBK_ERR_ARG;
    std::memset(&a, 0, sizeof(a));
    a.src = (const uint8_t *)p->src; a.dst = (uint8_t *)p->dst;
    a.pitch = (long long)p->pitch; a.frame_stride = (long long)p->frame_stride;
    a.plane_w = (int)p->plane_w; a.plane_h = (int)p->plane_h; a.n_frames = (int)p->n_frames;
    a.max_v = (1 << p->bit_depth) - 1; a.band_shift = (int)p->bit_depth - 5;
    a.params = reinterpret_cast<const DbkSaoCtb *>(params);
    a.params_stride = (int)params_stride; a.params_frame_stride = (long long)params_frame_stride;
    a.ctb_log2 = (int)ctb_log2;
    a.keep = keep; a.keep_stride = (int)keep_stride; a.keep_frame_stride = (long long)keep_frame_stride;
    return HEVCDBK_OK;
}

/* sao_args for CTBs of (1 << ctb_log2_w) x (1 << ctb_log2_h) samples: square, or twice as tall as wide (4:2:2 chroma) */
inline int sao_args_cf(const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride,
                       unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                       DbkSaoArgs &a, bool g4 = false)
{
    if (ctb_log2_h != ctb_log2_w && ctb_log2_h != ctb_log2_w + 1) return HEVCDBK_ERR_ARG;
    if (ctb_log2_h < 3 || ctb_log2_h > 6) return HEVCDBK_ERR_ARG;
    return sao_args(p, params, params_stride, params_frame_stride, ctb_log2_w, keep, keep_stride, keep_frame_stride, a, g4);
}

/* the two-launch form of deblocking + SAO: the deblocked planes go through ctx->dev_tmp (same pitch and frame stride).
 * The scratch plane is ONE buffer per context while the caller may hand in any stream: the previous user's SAO launch is
 * fenced by an event (ctx->tmp_ev) that the next user's stream waits for before it overwrites the scratch, and the buffer
 * is only re-allocated after that event has completed (two calls on different streams raced on it) */
inline int tmp_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *p, hipStream_t s, hevcdbk_device_planes &first,
                      hevcdbk_device_planes &second)
{
    const size_t bytes = (size_t)p->frame_stride * (p->n_frames ? p->n_frames - 1 : 0) + (size_t)p->pitch * p->plane_h;
    if (!ctx->tmp_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->tmp_ev, hipEventDisableTiming));
    if (ctx->tmp_used) {
        if (ctx->dev_tmp.cap < bytes) HIP_TRY(ctx, hipEventSynchronize(ctx->tmp_ev)); /* about to free it */
        else HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->tmp_ev, 0));
    }
    if (int rc = grow_device(ctx, ctx->dev_tmp, bytes)) return rc;
    first = *p;
    first.dst = ctx->dev_tmp.p;
    second = *p;
    second.src = ctx->dev_tmp.p;
    return HEVCDBK_OK;
}
/* the fence of one of the context's scratch buffers (dev_tmp / tmp_ev / tmp_used here, dev_sao in deblock_host_h265.cpp): an event
 * behind the last launch on s that touches the buffer.  Where the record itself fails there is nothing the next user could wait
 * for, so the stream is drained instead: the buffer is never left with work queued that its next user is not ordered behind.
 * failing: the call is returning an error already, and hevcdbk_last_error keeps speaking of that first failure */
inline int fence_scratch(hevcdbk_context *ctx, hipEvent_t ev, bool &used, hipStream_t s, bool failing = false)
{
    const hipError_t e = hipEventRecord(ev, s);
    if (e != hipSuccess) {
        if (!failing) (void)hip_ok(ctx, e, "hipEventRecord(scratch fence)");
        (void)hipStreamSynchronize(s);
        (void)hipGetLastError();
        return HEVCDBK_ERR_HIP;
    }
    used = true;
    return HEVCDBK_OK;
}
inline int tmp_done(hevcdbk_context *ctx, hipStream_t s, bool failing = false) { return fence_scratch(ctx, ctx->tmp_ev, ctx->tmp_used, s, failing); }

/* the two-launch form itself: deblock(first) filters the plane into the scratch plane, sao() -- its source now the scratch plane --
 * reads it from there; fenced for the next user whatever the launches returned: a deblocking launch that was enqueued writes the
 * scratch plane even when the SAO launch behind it failed, and the next call may come on another stream */
template <class Deblock, class Sao>
int through_scratch(hevcdbk_context *ctx, const hevcdbk_device_planes *p, hipStream_t s, DbkSaoArgs &sa, Deblock deblock, Sao sao)
{
    hevcdbk_device_planes first, second;
    if (int rc = tmp_planes(ctx, p, s, first, second)) return rc;
    int rc = deblock(first);
    if (rc == HEVCDBK_OK) {
        sa.src = (const uint8_t *)second.src;
        rc = sao();
    }
    const int rc2 = tmp_done(ctx, s, rc != HEVCDBK_OK);
    return rc ? rc : rc2;
}

/* the fused kernel takes plane p (every chroma format, one QP or a QP map: the conditions of deblock_sao_plane_h265) */
inline bool fused_can(const DbkH265Args &h, const DbkSaoArgs &sa, const hevcdbk_device_planes *p, int c_idx)
{
    return dbk_packed_h265_supports(h, (int)p->sample_bytes, c_idx != 0) && dbk_deblock_sao_supports(h.base, sa, (int)p->sample_bytes, c_idx != 0);
}

/* validates the slice / tile boundary operand of a plane whose SAO operands are `a` (before sao_square_params) and fills nx */
inline int nox_args(const hevcdbk_sao_borders *b, const DbkSaoArgs &a, DbkSaoNox &nx)
{
    if (!b->nox || b->stride < (unsigned)((a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2)) return HEVCDBK_ERR_ARG;
    nx.nox = b->nox;
    nx.stride = (int)b->stride;
    nx.frame_stride = (long long)b->frame_stride;
    return HEVCDBK_OK;
}

inline bool bad_fused(int fused) { return fused != HEVCDBK_FUSED_AUTO && fused != HEVCDBK_FUSED_OFF && fused != HEVCDBK_FUSED_ON; }

/* what the _sp entry asks of the plane beyond what the planar entries ask of a g4 plane of plane_w x plane_h: a chroma plane whose
 * rows hold the pairs */
inline int sp_plane_ok(const hevcdbk_device_planes *p)
{
    if (!p->is_chroma) return HEVCDBK_ERR_ARG;
    if (g4_kind(p->plane_w, p->plane_h) < 0) return HEVCDBK_ERR_DIMENSIONS;
    if (!bad_depth(p->bit_depth, p->sample_bytes) && p->pitch < 2 * (size_t)p->plane_w * p->sample_bytes) return HEVCDBK_ERR_ARG;
    return HEVCDBK_OK;
}

/* the SAO operands of a pair plane: what sp_plane_ok and, for one component of it, the _g4 SAO entry ask; square CTBs of 8..32 */
inline int sp_sao_args(const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params_cb, const hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                       size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                       const hevcdbk_sao_borders *borders, DbkSaoArgs &a, DbkSaoNox &nx)
{
    if (int rc = sp_plane_ok(p)) return rc;
    if (!params_cb || !params_cr || ctb_log2 < 3 || ctb_log2 > 5) return HEVCDBK_ERR_ARG;
    if (int rc = sao_args(p, params_cb, params_stride, params_frame_stride, ctb_log2, keep, keep_stride, keep_frame_stride, a, true)) return rc;
    if (borders)
        if (int rc = nox_args(borders, a, nx)) return rc;
    return HEVCDBK_OK;
}

} /* namespace dbkh */
