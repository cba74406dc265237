/*
 * deblock_host_sp.cpp -- C-ABI entries of deblocking + SAO in ONE kernel for semi-planar pictures: the plane of interleaved Cb / Cr
 * pairs alone (hevcdbk_h265_deblock_sao_device_sp_fused) and the Y plane with it in one launch (hevcdbk_h265_deblock_sao_device_nv12).
 * Where the fused kernels do not apply the entries run what the existing entries run, by calling them.  Operand checks:
 * deblock_host_args.h, shared with deblock_host_h265.cpp.
 */
#include "deblock_ctx.h"
#include "deblock_host_args.h"

using namespace dbkh;

namespace {

/* what a call says about its pair plane, checked in the order of hevcdbk_h265_deblock_sao_device_sp */
struct PairOperands {
    DbkSaoArgs sa;
    DbkSaoNox nx;
    DbkH265Args h;
    DbkSlOffs sl;
    int cr_qp_offset;
};

int pair_operands(const hevcdbk_device_planes *planes, unsigned qp, const hevcdbk_h265_params *prm, const hevcdbk_sao_plane_sp &sao,
                  const hevcdbk_sao_borders *borders, const hevcdbk_h265_slice_offsets *slice_offsets, PairOperands &o)
{
    if (int rc = sp_sao_args(planes, sao.params_cb, sao.params_cr, sao.params_stride, sao.params_frame_stride, sao.ctb_log2, sao.keep,
                             sao.keep_stride, sao.keep_frame_stride, borders, o.sa, o.nx))
        return rc;
    if (int rc = h265_args(planes, 1, qp, prm, o.h, true)) return rc; /* h.c_qp_offset = cb_qp_offset: the even samples */
    o.cr_qp_offset = prm ? prm->cr_qp_offset : 0;
    return sl_args_g4(slice_offsets, planes, 1, HEVCDBK_CHROMA_420, o.h, o.sl);
}

/* the pair plane once its operands are checked and the device is bound: the fused kernel (can, and not switched off), else the
 * existing entry's two launches */
int pair_plane(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp, const hevcdbk_h265_params *prm,
               const hevcdbk_sao_plane_sp &sao, const PairOperands &o, bool can, int fused, const hevcdbk_sao_borders *borders,
               const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    if (can && fused != HEVCDBK_FUSED_OFF) {
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
        const hipError_t e = dbk_launch_deblock_sao_h265_sp(o.h, o.sa, reinterpret_cast<const DbkSaoCtb *>(sao.params_cr), o.sl, o.cr_qp_offset,
                                                            (int)planes->sample_bytes, s, borders ? &o.nx : nullptr);
        return hip_ok(ctx, e, "fused deblocking + SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    }
    return hevcdbk_h265_deblock_sao_device_sp(ctx, planes, qp, prm, sao.params_cb, sao.params_cr, sao.params_stride, sao.params_frame_stride,
                                              sao.ctb_log2, sao.keep, sao.keep_stride, sao.keep_frame_stride, HEVCDBK_FUSED_OFF, borders,
                                              slice_offsets, hip_stream);
}

} /* namespace */

extern "C" {

int hevcdbk_h265_deblock_sao_device_sp_fused(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp,
                                             const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params_cb, const hevcdbk_sao_ctb *params_cr,
                                             unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep,
                                             unsigned keep_stride, size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                             const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    if (!ctx || !planes || bad_fused(fused)) return HEVCDBK_ERR_ARG;
    const hevcdbk_sao_plane_sp sao = {params_cb, params_cr, params_stride, params_frame_stride, ctb_log2, keep, keep_stride, keep_frame_stride};
    PairOperands o;
    if (int rc = pair_operands(planes, qp, prm, sao, borders, slice_offsets, o)) return rc;
    const bool can = dbk_deblock_sao_sp_supports(o.h, o.sa, (int)planes->sample_bytes);
    if (fused == HEVCDBK_FUSED_ON && !can) return HEVCDBK_ERR_UNSUPPORTED; /* before any launch */
    if (int rc = bind(ctx)) return rc;
    return pair_plane(ctx, planes, qp, prm, sao, o, can, fused, borders, slice_offsets, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_nv12(hevcdbk_context *ctx, const hevcdbk_device_planes *luma, const hevcdbk_device_planes *pairs, unsigned qp,
                                         const hevcdbk_h265_params *prm, const hevcdbk_sao_plane_cf *sao_luma,
                                         const hevcdbk_sao_plane_sp *sao_pairs, int fused, const hevcdbk_sao_borders *borders,
                                         const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    if (!ctx || !luma || !pairs || !sao_luma || !sao_pairs || bad_fused(fused)) return HEVCDBK_ERR_ARG;
    /* the luma plane as the _planes_g4 entry checks it */
    DbkH265Args hy;
    DbkSaoArgs say;
    DbkSaoNox nxy;
    DbkSlOffs sly;
    if (int rc = sao_args_cf(luma, sao_luma->params, sao_luma->params_stride, sao_luma->params_frame_stride, sao_luma->ctb_log2_w,
                             sao_luma->ctb_log2_h, sao_luma->keep, sao_luma->keep_stride, sao_luma->keep_frame_stride, say, true))
        return rc;
    if (int rc = h265_args_cf(luma, 0, HEVCDBK_CHROMA_420, qp, prm, hy, true)) return rc;
    if (borders)
        if (int rc = nox_args(borders, say, nxy)) return rc;
    if (int rc = sl_args_g4(slice_offsets, luma, 0, HEVCDBK_CHROMA_420, hy, sly)) return rc;
    /* the pair plane as the _sp entries check it */
    PairOperands o;
    if (int rc = pair_operands(pairs, qp, prm, *sao_pairs, borders, slice_offsets, o)) return rc;
    /* one picture */
    if (pairs->n_frames != luma->n_frames || pairs->sample_bytes != luma->sample_bytes || pairs->bit_depth != luma->bit_depth ||
        pairs->plane_w * 2 != luma->plane_w || pairs->plane_h * 2 != luma->plane_h)
        return HEVCDBK_ERR_ARG;
    if (sao_luma->ctb_log2_h != sao_luma->ctb_log2_w || sao_pairs->ctb_log2 + 1 != sao_luma->ctb_log2_w) return HEVCDBK_ERR_ARG;
    const int sb = (int)luma->sample_bytes;
    const bool can_y = fused_can(hy, say, luma, 0), can_c = dbk_deblock_sao_sp_supports(o.h, o.sa, sb);
    if (fused == HEVCDBK_FUSED_ON && !(can_y && can_c)) return HEVCDBK_ERR_UNSUPPORTED; /* before any launch */
    /* one launch: both fused kernels apply and both planes have one kind of QP (the luma body and the pair body each test theirs,
     * but the picture has one QP map or none) */
    const bool one = fused != HEVCDBK_FUSED_OFF && can_y && can_c && (hy.base.qp_map != nullptr) == (o.h.base.qp_map != nullptr);
    if (int rc = bind(ctx)) return rc;
    if (one) {
        hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
        const DbkH265Args h[2] = {hy, o.h};
        const DbkSaoArgs sa[2] = {say, o.sa};
        const DbkSaoNox nx[2] = {nxy, o.nx};
        const hipError_t e = dbk_launch_deblock_sao_h265_nv12(h, sa, reinterpret_cast<const DbkSaoCtb *>(sao_pairs->params_cr), sly, o.cr_qp_offset,
                                                              sb, s, borders ? nx : nullptr);
        return hip_ok(ctx, e, "fused deblocking + SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    }
    /* plane by plane, each in its best available form */
    if (int rc = hevcdbk_h265_deblock_sao_device_planes_g4(ctx, luma, 1, HEVCDBK_CHROMA_420, qp, prm, sao_luma, fused, borders, slice_offsets,
                                                           hip_stream))
        return rc;
    return pair_plane(ctx, pairs, qp, prm, *sao_pairs, o, can_c, fused, borders, slice_offsets, hip_stream);
}

} /* extern "C" */
