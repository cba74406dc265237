/*
 * deblock_host_h265.cpp -- C-ABI entries of the spec-exact mode (ITU-T H.265 clause 8.7.2: bS derivation, block filter,
 * host-frame operator) and of sample adaptive offset (clause 8.7.3).  Context and shared helpers: deblock_ctx.h; the validation of
 * the operands, shared with deblock_host_sp.cpp: deblock_host_args.h.
 */
#include <chrono>
#include <cstring>

#include "deblock_ctx.h"
#include "deblock_host_args.h"
#ifdef HEVCDBK_DIAG
#include "hevcdbk_diag.h"
#endif

using namespace dbkh;

extern "C" {

/* ---- spec-exact mode (H.265 clause 8.7.2) ------------------------------------------------------------------ */

size_t hevcdbk_h265_num_vert_bs(unsigned w, unsigned h) { return (size_t)(w / 8 + 1) * (h / 4); }
size_t hevcdbk_h265_num_hor_bs(unsigned w, unsigned h) { return (size_t)(h / 8 + 1) * (w / 4); }

namespace {

/* the operand of a plane's launches.  g4 (the call holds a g4 plane): as sl_args_g4 for every plane of the call; else the caller's
 * array, the call's own pair staying in h (the _sl kernels do not read it) */
int slice_args(const hevcdbk_h265_slice_offsets *so, const hevcdbk_device_planes *p, int c_idx, int cf, bool g4, DbkH265Args &h, DbkSlOffs &sl)
{
    return g4 || !so ? sl_args_g4(so, p, c_idx, cf, h, sl) : sl_args(so, p, c_idx, cf, sl);
}

/* the kernel generation a plane runs: a g4 plane (where the entry takes one) the _g4 kernels, with kNoSlOffs when there is no
 * per-slice operand; any other plane the _sl kernels with the operand and the _cf / _nox kernels without it -- never _sl kernels on
 * an empty array */
enum class Gen { CF, SL, G4 };
Gen plane_gen(const hevcdbk_device_planes *p, const hevcdbk_h265_slice_offsets *so, bool g4)
{
    if (g4 && g4_kind(p->plane_w, p->plane_h) == 1) return Gen::G4;
    return so ? Gen::SL : Gen::CF;
}

/* kernel_variant split into the kernel (HEVCDBK_KERNEL_*) and DbkArgs::map_override; HEVCDBK_ERR_ARG for a selector that does not
 * exist.  diag_maps: the diagnostic build's maps as well (_cf generation only: the _sl / _g4 / _sp kernels have the product's maps) */
int check_variant(int &variant, int &map_override, bool diag_maps)
{
    const int map = variant & HEVCDBK_MAP_MASK; /* as in dbkh::launch */
    variant &= ~HEVCDBK_MAP_MASK;
    bool known = map == HEVCDBK_MAP_AUTO || map == HEVCDBK_MAP_ROWS || map == HEVCDBK_MAP_LINEAR;
#ifdef HEVCDBK_DIAG
    known = known || (diag_maps && (map == HEVCDBK_DIAG_MAP_TILES || map == HEVCDBK_DIAG_MAP_STRIPE || map == HEVCDBK_DIAG_MAP_PIPE || map == HEVCDBK_DIAG_MAP_GROUP));
#endif
    if (!known || (variant != HEVCDBK_KERNEL_PACKED && variant != HEVCDBK_KERNEL_GENERIC && variant != HEVCDBK_KERNEL_AUTO)) return HEVCDBK_ERR_ARG;
    map_override = map >> 8; /* ROWS 1, LINEAR 2, the diagnostic maps 3..6 */
    return HEVCDBK_OK;
}

/* the deblocking launch of plane c_idx of a picture in chroma format cf: the packed kernel where it applies (and is not ruled out),
 * else the 32-bit one, of generation gen (sl: its per-slice operand, not read by Gen::CF) */
int launch_h265(hevcdbk_context *ctx, const DbkH265Args &h0, const DbkSlOffs &sl, Gen gen, int sample_bytes, int c_idx, int cf, int variant,
                hipStream_t s)
{
    int map_override;
    if (int rc = check_variant(variant, map_override, gen == Gen::CF)) return rc;
    DbkH265Args h = h0;
    h.base.map_override = map_override;
    const bool chroma = c_idx != 0;
    const bool pack = dbk_packed_h265_supports(h, sample_bytes, chroma);
    if (variant == HEVCDBK_KERNEL_PACKED && !pack) return HEVCDBK_ERR_UNSUPPORTED;
    const bool packed = pack && variant != HEVCDBK_KERNEL_GENERIC;
    hipError_t e;
    if (gen == Gen::G4) /* chroma planes only */
        e = packed ? dbk_launch_packed_h265_g4(h, sl, sample_bytes, cf, s) : dbk_launch_h265_g4(h, sl, sample_bytes, cf, s);
    else if (gen == Gen::SL) /* luma is format 0 to the 32-bit kernel, format 1 (which does not enter luma) to the packed ones */
        e = packed ? dbk_launch_packed_h265_sl(h, sl, sample_bytes, chroma, chroma ? cf : 1, s) : dbk_launch_h265_sl(h, sl, sample_bytes, chroma ? cf : 0, s);
    else if (chroma && cf != HEVCDBK_CHROMA_420)
        /* 4:2:2 / 4:4:4 chroma: the packed kernels (one QP: the 4:2:0 kernels with QpC folded into their scalar tc; a QP map: the
         * format's own instantiations), the 32-bit kernel for every operand kind */
        e = packed ? dbk_launch_packed_h265_cf(h, sample_bytes, true, cf, s) : dbk_launch_h265_cf(h, sample_bytes, cf, s);
    else
        e = packed ? dbk_launch_packed_h265(h, sample_bytes, chroma, s) : dbk_launch_h265(h, sample_bytes, chroma, s);
    return hip_ok(ctx, e, "kernel launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* the bS derivation entries.  g4: chroma planes of multiples of 4 (the _g4 entry) */
int derive_bs(hevcdbk_context *ctx, const hevcdbk_h265_units *u, unsigned width, unsigned height, int cf, bool g4, uint8_t *vert_bs4,
              uint8_t *hor_bs4, uint8_t *chroma_vert_bs4, uint8_t *chroma_hor_bs4, void *hip_stream)
{
    if (!ctx || !u || !u->flags || !u->mv0 || !u->mv1 || !u->ref0 || !u->ref1 || !vert_bs4 || !hor_bs4) return HEVCDBK_ERR_ARG;
    if (cf < HEVCDBK_CHROMA_400 || cf > HEVCDBK_CHROMA_444) return HEVCDBK_ERR_ARG;
    if ((chroma_vert_bs4 != nullptr) != (chroma_hor_bs4 != nullptr)) return HEVCDBK_ERR_ARG;
    if (cf == HEVCDBK_CHROMA_400 && chroma_vert_bs4) return HEVCDBK_ERR_ARG;
    if (width == 0 || height == 0 || width % 8 != 0 || height % 8 != 0) return HEVCDBK_ERR_DIMENSIONS;
    if (chroma_vert_bs4) {
        const unsigned cw = width / sub_w(cf), ch = height / sub_h(cf);
        /* _g4: multiples of 4 in every format, what is left to ask is "at least 8".  The others: the chroma planes' 8-sample grid;
         * the codes are the generations' own (4:2:0 entry: a dimension error; _cf: 4:2:2 with width % 16 != 0 an argument error) */
        if (g4 ? g4_kind(cw, ch) < 0 : (cw % 8 != 0 || ch % 8 != 0)) return g4 || cf == HEVCDBK_CHROMA_420 ? HEVCDBK_ERR_DIMENSIONS : HEVCDBK_ERR_ARG;
    }
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const bool gather = cf == HEVCDBK_CHROMA_420; /* 4:2:0 chroma arrays come out of the luma launch (its gathers divide with floor) */
    hipError_t e = dbk_launch_h265_bs(u->flags, u->mv0, u->mv1, u->ref0, u->ref1, (int)width, (int)height, vert_bs4, hor_bs4,
                                      gather ? chroma_vert_bs4 : nullptr, gather ? chroma_hor_bs4 : nullptr, s);
    if (e == hipSuccess && chroma_vert_bs4 && !gather)
        e = dbk_launch_h265_chroma_bs_cf(vert_bs4, hor_bs4, (int)width, (int)height, cf, chroma_vert_bs4, chroma_hor_bs4, s);
    return hip_ok(ctx, e, "bS derivation launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* the block filter entries.  g4: the entry takes a g4 plane */
int filter_plane(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int cf, unsigned qp, const hevcdbk_h265_params *params,
                 int kernel_variant, const hevcdbk_h265_slice_offsets *so, bool g4, void *hip_stream)
{
    if (!ctx) return HEVCDBK_ERR_ARG;
    DbkH265Args h;
    if (int rc = h265_args_cf(planes, c_idx, cf, qp, params, h, g4)) return rc;
    const Gen gen = plane_gen(planes, so, g4);
    DbkSlOffs sl;
    if (int rc = slice_args(so, planes, c_idx, cf, gen == Gen::G4, h, sl)) return rc;
    if (gen != Gen::CF) { /* the _sl and _g4 generations check kernel_variant before they bind the device, the _cf one after (in launch_h265) */
        int variant = kernel_variant, map_override;
        if (int rc = check_variant(variant, map_override, false)) return rc;
        if (variant == HEVCDBK_KERNEL_PACKED && !dbk_packed_h265_supports(h, (int)planes->sample_bytes, c_idx != 0)) return HEVCDBK_ERR_UNSUPPORTED;
    }
    if (int rc = bind(ctx)) return rc;
    return launch_h265(ctx, h, sl, gen, (int)planes->sample_bytes, c_idx, cf, kernel_variant, hip_stream ? (hipStream_t)hip_stream : ctx->compute);
}

} /* namespace */

int hevcdbk_h265_derive_bs_device(hevcdbk_context *ctx, const hevcdbk_h265_units *u, unsigned width, unsigned height,
                                  uint8_t *vert_bs4, uint8_t *hor_bs4, uint8_t *chroma_vert_bs4, uint8_t *chroma_hor_bs4,
                                  void *hip_stream)
{
    return derive_bs(ctx, u, width, height, HEVCDBK_CHROMA_420, false, vert_bs4, hor_bs4, chroma_vert_bs4, chroma_hor_bs4, hip_stream);
}

int hevcdbk_h265_derive_bs_device_cf(hevcdbk_context *ctx, const hevcdbk_h265_units *u, unsigned width, unsigned height,
                                     int chroma_format_idc, uint8_t *vert_bs4, uint8_t *hor_bs4, uint8_t *chroma_vert_bs4,
                                     uint8_t *chroma_hor_bs4, void *hip_stream)
{
    return derive_bs(ctx, u, width, height, chroma_format_idc, false, vert_bs4, hor_bs4, chroma_vert_bs4, chroma_hor_bs4, hip_stream);
}

int hevcdbk_h265_derive_bs_device_g4(hevcdbk_context *ctx, const hevcdbk_h265_units *u, unsigned width, unsigned height,
                                     int chroma_format_idc, uint8_t *vert_bs4, uint8_t *hor_bs4, uint8_t *chroma_vert_bs4,
                                     uint8_t *chroma_hor_bs4, void *hip_stream)
{
    return derive_bs(ctx, u, width, height, chroma_format_idc, true, vert_bs4, hor_bs4, chroma_vert_bs4, chroma_hor_bs4, hip_stream);
}

int hevc_deblocking_filter_h265_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, unsigned qp,
                                       const hevcdbk_h265_params *params, int kernel_variant, void *hip_stream)
{
    return filter_plane(ctx, planes, c_idx, HEVCDBK_CHROMA_420, qp, params, kernel_variant, nullptr, false, hip_stream);
}

int hevcdbk_h265_filter_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int chroma_format_idc,
                                          unsigned qp, const hevcdbk_h265_params *params, int kernel_variant, void *hip_stream)
{
    return filter_plane(ctx, planes, c_idx, chroma_format_idc, qp, params, kernel_variant, nullptr, false, hip_stream);
}

int hevcdbk_h265_filter_device_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int chroma_format_idc, unsigned qp,
                                  const hevcdbk_h265_params *params, int kernel_variant, const hevcdbk_h265_slice_offsets *slice_offsets,
                                  void *hip_stream)
{
    return filter_plane(ctx, planes, c_idx, chroma_format_idc, qp, params, kernel_variant, slice_offsets, false, hip_stream);
}

int hevcdbk_h265_filter_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int chroma_format_idc, unsigned qp,
                                  const hevcdbk_h265_params *params, int kernel_variant, const hevcdbk_h265_slice_offsets *slice_offsets,
                                  void *hip_stream)
{
    return filter_plane(ctx, planes, c_idx, chroma_format_idc, qp, params, kernel_variant, slice_offsets, true, hip_stream);
}

int hevc_deblocking_filter_h265(hevcdbk_context *ctx, hevcdbk_frame *frame, const hevcdbk_h265_units *units,
                                const hevcdbk_bs *bs4, const hevcdbk_qp *qp, const hevcdbk_h265_params *params,
                                hevcdbk_timing *timing)
{
    return hevcdbk_h265_filter_frame_cf(ctx, frame, HEVCDBK_CHROMA_420, units, bs4, qp, params, timing);
}

int hevcdbk_h265_filter_frame_cf(hevcdbk_context *ctx, hevcdbk_frame *frame, int chroma_format_idc, const hevcdbk_h265_units *units,
                                   const hevcdbk_bs *bs4, const hevcdbk_qp *qp, const hevcdbk_h265_params *params,
                                   hevcdbk_timing *timing)
{
    const int cf = chroma_format_idc;
    if (!ctx || !frame || !qp || !frame->plane[0] || (units != nullptr) == (bs4 != nullptr)) return HEVCDBK_ERR_ARG;
    if (cf < HEVCDBK_CHROMA_400 || cf > HEVCDBK_CHROMA_444) return HEVCDBK_ERR_ARG;
    if (bad_depth(frame->bit_depth, frame->sample_bytes)) return HEVCDBK_ERR_ARG;
    const unsigned W = frame->width, H = frame->height, sb = frame->sample_bytes;
    if (W == 0 || H == 0 || W % 8 != 0 || H % 8 != 0) return HEVCDBK_ERR_DIMENSIONS;
    const bool chroma = frame->plane[1] && frame->plane[2];
    if (cf == HEVCDBK_CHROMA_400 && (frame->plane[1] || frame->plane[2])) return HEVCDBK_ERR_ARG;
    const unsigned cw = cf ? W / sub_w(cf) : 0, ch = cf ? H / sub_h(cf) : 0;
    if (chroma && (cw % 8 != 0 || ch % 8 != 0)) return cf == HEVCDBK_CHROMA_420 ? HEVCDBK_ERR_DIMENSIONS : HEVCDBK_ERR_ARG;
    const int npl = chroma ? 3 : 1;
    const unsigned pw[3] = {W, cw, cw}, ph[3] = {H, ch, ch};
    for (int i = 0; i < npl; i++)
        if (frame->pitch[i] < (size_t)pw[i] * sb) return HEVCDBK_ERR_ARG;
    const size_t nv = hevcdbk_h265_num_vert_bs(W, H), nh = hevcdbk_h265_num_hor_bs(W, H);
    const size_t ncv = chroma ? hevcdbk_h265_num_vert_bs(cw, ch) : 0, nch = chroma ? hevcdbk_h265_num_hor_bs(cw, ch) : 0;
    if (bs4) {
        if (!bs4->vert || !bs4->hor) return HEVCDBK_ERR_ARG;
        if (bs4->n_vert != nv || bs4->n_hor != nh) return HEVCDBK_ERR_BS_SIZE;
    } else if (!units->flags || !units->mv0 || !units->mv1 || !units->ref0 || !units->ref1) {
        return HEVCDBK_ERR_ARG;
    }
    size_t map_rows = 0;
    if (qp->map) {
        if (qp->ctu_log2 < 3 || qp->ctu_log2 > 8 || qp->map_stride < ((W + (1u << qp->ctu_log2) - 1) >> qp->ctu_log2))
            return HEVCDBK_ERR_ARG;
        map_rows = (H + (1u << qp->ctu_log2) - 1) >> qp->ctu_log2;
    }
    if (int rc = bind(ctx)) return rc;
    GpuDrain drain{ctx}; /* every return below that is not HEVCDBK_OK waits for the GPU */

    const FrameLayout L = frame_layout(npl, pw, ph, sb);
    if (int rc = grow_pinned(ctx, ctx->pin[0], L.frame_bytes)) return rc;
    if (int rc = grow_device(ctx, ctx->dev[0], L.frame_bytes)) return rc;
    if (int rc = grow_device(ctx, ctx->dev_bs, nv + nh + ncv + nch)) return rc;
    ctx->bs_default_at = nullptr; /* dev_bs no longer holds the reference's default pattern */
    if (qp->map)
        if (int rc = grow_device(ctx, ctx->dev_map, map_rows * qp->map_stride)) return rc;
    const size_t U = (size_t)(W / 4) * (H / 4);
    if (units)
        if (int rc = grow_device(ctx, ctx->dev_units, 18 * U)) return rc;
    uint8_t *dbs = (uint8_t *)ctx->dev_bs.p, *dun = (uint8_t *)ctx->dev_units.p;
    uint8_t *dmap = qp->map ? (uint8_t *)ctx->dev_map.p : nullptr;
    hipStream_t s = ctx->compute;
    hipEvent_t *ev = ctx->ev;

    /* The frame's way in and out (round 4, as hevc_deblocking_filter's large-frame path): on a large-BAR device the staging crew
     * writes the caller's rows straight into fine-grained HBM through the BAR and the kernels store their results straight into
     * the page-locked ring, from which the crew copies them back -- no DMA in either direction; elsewhere ring + DMA both ways,
     * the ring filled and emptied by the crew.  Not cut into strips: the bS derivation wants the whole picture's units first. */
    const auto wall0 = std::chrono::steady_clock::now();
    uint8_t *const ring = (uint8_t *)ctx->pin[0].p;
    uint8_t *const dpush = push_buffer(ctx, L.frame_bytes);
    uint8_t *const din = dpush ? dpush : (uint8_t *)ctx->dev[0].p;    /* what the kernels read */
    uint8_t *const dout = dpush ? ring : (uint8_t *)ctx->dev[0].p;    /* what they write */
    if (int rc = crew_copy_frame(ctx, frame, L, dpush ? dpush : ring, false, dpush != nullptr)) return rc;
    const double push_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count();
    HIP_TRY(ctx, hipEventRecord(ev[0], s));
    if (!dpush) HIP_TRY(ctx, hipMemcpyAsync(ctx->dev[0].p, ring, L.frame_bytes, hipMemcpyHostToDevice, s));
    if (dmap) HIP_TRY(ctx, hipMemcpyAsync(dmap, qp->map, map_rows * qp->map_stride, hipMemcpyHostToDevice, s));
    if (units) {
        /* device layout: ref0 | ref1 | mv0 | mv1 | flags (descending alignment) */
        HIP_TRY(ctx, hipMemcpyAsync(dun, units->ref0, 4 * U, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(dun + 4 * U, units->ref1, 4 * U, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(dun + 8 * U, units->mv0, 4 * U, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(dun + 12 * U, units->mv1, 4 * U, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(dun + 16 * U, units->flags, 2 * U, hipMemcpyHostToDevice, s));
    } else {
        HIP_TRY(ctx, hipMemcpyAsync(dbs, bs4->vert, nv, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(dbs + nv, bs4->hor, nh, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ctx, hipEventRecord(ev[1], s));
    uint8_t *dcv = chroma ? dbs + nv + nh : nullptr, *dch = chroma ? dbs + nv + nh + ncv : nullptr;
    hipError_t e;
    if (cf == HEVCDBK_CHROMA_420 || !chroma) {
        if (units) e = dbk_launch_h265_bs(dun + 16 * U, dun + 8 * U, dun + 12 * U, dun, dun + 4 * U, (int)W, (int)H, dbs, dbs + nv, dcv, dch, s);
        else e = chroma ? dbk_launch_h265_chroma_bs(dbs, dbs + nv, (int)W, (int)H, dcv, dch, s) : hipSuccess;
    } else {
        e = units ? dbk_launch_h265_bs(dun + 16 * U, dun + 8 * U, dun + 12 * U, dun, dun + 4 * U, (int)W, (int)H, dbs, dbs + nv, nullptr,
                                       nullptr, s)
                  : hipSuccess;
        if (e == hipSuccess) e = dbk_launch_h265_chroma_bs_cf(dbs, dbs + nv, (int)W, (int)H, cf, dcv, dch, s);
    }
    if (!hip_ok(ctx, e, "bS derivation launch")) return HEVCDBK_ERR_HIP;
    for (int i = 0; i < npl; i++) {
        hevcdbk_device_planes p;
        std::memset(&p, 0, sizeof(p));
        p.src = din + L.plane_off[i];
        p.dst = dout + L.plane_off[i];
        p.pitch = L.row_bytes[i]; p.frame_stride = L.plane_bytes[i]; p.n_frames = 1;
        p.plane_w = pw[i]; p.plane_h = ph[i]; p.bit_depth = frame->bit_depth; p.sample_bytes = sb;
        p.is_chroma = i != 0;
        p.vert_bs = i == 0 ? dbs : dcv;
        p.hor_bs = i == 0 ? dbs + nv : dch;
        p.qp_map = dmap; p.qp_map_stride = qp->map_stride; p.ctu_log2 = qp->ctu_log2;
        DbkH265Args h;
        if (int rc = h265_args(&p, i, qp->qp, params, h)) return rc;
        if (int rc = launch_h265(ctx, h, kNoSlOffs, Gen::CF, (int)sb, i, cf, HEVCDBK_KERNEL_AUTO, s)) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ev[2], s));
    if (!dpush) HIP_TRY(ctx, hipMemcpyAsync(ring, ctx->dev[0].p, L.frame_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(ev[3], s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    if (int rc = crew_copy_frame(ctx, frame, L, ring, true, false)) return rc;
    const auto wall1 = std::chrono::steady_clock::now();
    if (timing) {
        float a = 0.f, b = 0.f, c = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(ctx, hipEventElapsedTime(&b, ev[1], ev[2]));
        HIP_TRY(ctx, hipEventElapsedTime(&c, ev[2], ev[3]));
        /* exec: with the BAR path the download is the kernels' own stores, inside it; copy: uploads of bS / units / map (+ the frame: DMA, or
         * the crew's writes) */
        set_timing(timing, b * 1e-3, (a + c) * 1e-3 + (dpush ? push_s : 0.0), std::chrono::duration<double>(wall1 - wall0).count());
    }
    drain.ok = true;
    return HEVCDBK_OK;
}

/* ---- sample adaptive offset (H.265 clause 8.7.3) ------------------------------------------------------------- */

static_assert(sizeof(hevcdbk_sao_ctb) == sizeof(DbkSaoCtb) && sizeof(DbkSaoCtb) == 6, "SAO CTB entry layout");

namespace {

/* one plane: the fused kernel where it applies (and is not switched off), else the two launches */
int deblock_sao_plane(hevcdbk_context *ctx, const hevcdbk_device_planes *p, unsigned qp, const hevcdbk_tables *tables, DbkArgs &da,
                      DbkSaoArgs &sa, int fused, hipStream_t s)
{
    const int sb = (int)p->sample_bytes;
    const bool chroma = p->is_chroma != 0, can = dbk_deblock_sao_supports(da, sa, sb, chroma);
    if (fused == HEVCDBK_FUSED_ON && !can) return HEVCDBK_ERR_UNSUPPORTED;
    if (can && fused != HEVCDBK_FUSED_OFF)
        return hip_ok(ctx, dbk_launch_deblock_sao(da, sa, sb, chroma, s), "fused deblocking + SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    return through_scratch(
        ctx, p, s, sa,
        [&](const hevcdbk_device_planes &first) {
            if (int rc = planes_to_args(&first, qp, tables, da)) return rc;
            return launch(ctx, da, sb, chroma, HEVCDBK_KERNEL_AUTO, s);
        },
        [&] { return hip_ok(ctx, dbk_launch_sao(sa, sb, s), "SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP; });
}

/* 4:2:2 chroma planes (ctb_log2_h[i] = sa[i].ctb_log2 + 1): their SAO parameters rewritten as those of square CTBs into the
 * context's scratch (dbk_launch_sao_rows_x2), so that every kernel after this sees square CTBs.  Like dev_tmp, the scratch is
 * fenced by an event: the next user waits for the last launch that touched it (sao_done), whatever that launch and the ones
 * behind it returned */
/* the bytes of a 4:2:2 chroma plane's rows of CTBs, doubled like the parameters (dbk_launch_sao_nox_rows_x2) */
size_t nox_x2_bytes(const DbkSaoArgs &a, const DbkSaoNox &nx)
{
    const size_t cols = (size_t)((a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2), rows = (size_t)((a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2);
    return cols * rows * (nx.frame_stride ? (size_t)a.n_frames : 1);
}

int sao_done(hevcdbk_context *ctx, hipStream_t s, bool failing = false);

/* nx (may be NULL): the planes' slice / tile boundary bytes, rewritten with the parameters into the same scratch.  A launch that
 * fails after another was enqueued leaves the scratch fenced: the enqueued one writes it */
int sao_square_params(hevcdbk_context *ctx, DbkSaoArgs *sa, const unsigned *ctb_log2_h, unsigned n, hipStream_t s, DbkSaoNox *nx = nullptr)
{
    size_t entries = 0, nox_bytes = 0;
    for (unsigned i = 0; i < n; i++)
        if (ctb_log2_h[i] != (unsigned)sa[i].ctb_log2) {
            entries += dbk_sao_rows_x2_entries(sa[i]);
            if (nx) nox_bytes += nox_x2_bytes(sa[i], nx[i]);
        }
    if (entries == 0) return HEVCDBK_OK;
    const size_t bytes = entries * sizeof(DbkSaoCtb) + nox_bytes;
    if (!ctx->sao_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->sao_ev, hipEventDisableTiming));
    if (ctx->sao_used) {
        if (ctx->dev_sao.cap < bytes) HIP_TRY(ctx, hipEventSynchronize(ctx->sao_ev)); /* about to free it */
        else HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->sao_ev, 0));
    }
    if (int rc = grow_device(ctx, ctx->dev_sao, bytes)) return rc;
    DbkSaoCtb *dst = (DbkSaoCtb *)ctx->dev_sao.p;
    uint8_t *nox_dst = (uint8_t *)ctx->dev_sao.p + entries * sizeof(DbkSaoCtb);
    for (unsigned i = 0; i < n; i++)
        if (ctb_log2_h[i] != (unsigned)sa[i].ctb_log2) {
            if (nx) {
                const size_t nb = nox_x2_bytes(sa[i], nx[i]);
                if (!hip_ok(ctx, dbk_launch_sao_nox_rows_x2(sa[i], nx[i], nox_dst, s), "SAO border launch")) {
                    (void)sao_done(ctx, s, true);
                    return HEVCDBK_ERR_HIP;
                }
                nox_dst += nb;
            }
            const size_t k = dbk_sao_rows_x2_entries(sa[i]);
            if (!hip_ok(ctx, dbk_launch_sao_rows_x2(sa[i], dst, s), "SAO parameter launch")) {
                (void)sao_done(ctx, s, true);
                return HEVCDBK_ERR_HIP;
            }
            dst += k;
        }
    return HEVCDBK_OK;
}
int sao_done(hevcdbk_context *ctx, hipStream_t s, bool failing)
{
    if (!ctx->sao_ev) return HEVCDBK_OK; /* no 4:2:2 plane ever used the scratch */
    return fence_scratch(ctx, ctx->sao_ev, ctx->sao_used, s, failing);
}

/* what a deblocking + SAO call says about its picture, whichever generation of the C ABI it came through */
struct Picture {
    int cf;                                   /* chroma_format_idc (4:2:0 for the original entries) */
    unsigned qp;
    const hevcdbk_h265_params *prm;
    int fused;
    const hevcdbk_sao_borders *borders;       /* may be NULL: the kernels without the operand */
    const hevcdbk_h265_slice_offsets *so;     /* may be NULL: likewise */
    bool first_gen;                           /* the original 4:2:0 entries: square CTBs, and HEVCDBK_FUSED_ON is looked at after the bind */
    bool g4;                                  /* a _g4 entry that was given a g4 plane */
};

/* validates the operands of plane c_idx and fills what its launches take */
int plane_operands(const Picture &pic, const hevcdbk_device_planes *p, int c_idx, const hevcdbk_sao_plane_cf &sao, DbkH265Args &h, DbkSaoArgs &sa,
                   DbkSaoNox &nx, DbkSlOffs &sl)
{
    if (int rc = pic.first_gen ? sao_args(p, sao.params, sao.params_stride, sao.params_frame_stride, sao.ctb_log2_w, sao.keep, sao.keep_stride,
                                          sao.keep_frame_stride, sa)
                               : sao_args_cf(p, sao.params, sao.params_stride, sao.params_frame_stride, sao.ctb_log2_w, sao.ctb_log2_h, sao.keep,
                                             sao.keep_stride, sao.keep_frame_stride, sa, pic.g4))
        return rc;
    if (int rc = h265_args_cf(p, c_idx, pic.cf, pic.qp, pic.prm, h, pic.g4)) return rc;
    if (pic.borders)
        if (int rc = nox_args(pic.borders, sa, nx)) return rc;
    return slice_args(pic.so, p, c_idx, pic.cf, pic.g4, h, sl);
}

/* deblocking + SAO of one plane (square CTBs: after sao_square_params): the fused kernel where it applies (and is not switched
 * off), else the two launches through the context's scratch plane; the kernels of the plane's generation */
int deblock_sao_plane_h265(hevcdbk_context *ctx, const Picture &pic, const hevcdbk_device_planes *p, int c_idx, DbkH265Args &h, DbkSaoArgs &sa,
                           const DbkSlOffs &sl, const DbkSaoNox *nx, hipStream_t s)
{
    const Gen gen = plane_gen(p, pic.so, pic.g4);
    const int sb = (int)p->sample_bytes, cf = c_idx != 0 ? pic.cf : 1; /* the format does not enter luma */
    const bool can = fused_can(h, sa, p, c_idx);
    if (pic.fused == HEVCDBK_FUSED_ON && !can) return HEVCDBK_ERR_UNSUPPORTED;
    if (can && pic.fused != HEVCDBK_FUSED_OFF) {
        const hipError_t e = gen == Gen::G4   ? dbk_launch_deblock_sao_h265_g4(h, sa, sl, sb, pic.cf, s, nx)
                             : gen == Gen::SL ? dbk_launch_deblock_sao_h265_sl(h, sa, sl, sb, c_idx != 0, cf, s, nx)
                                              : dbk_launch_deblock_sao_h265_cf(h, sa, sb, c_idx != 0, cf, s, nx);
        return hip_ok(ctx, e, "fused deblocking + SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    }
    const int tc_off = h.tc_off, beta_off = h.beta_off;
    return through_scratch(
        ctx, p, s, sa,
        [&](const hevcdbk_device_planes &first) {
            if (int rc = h265_args(&first, c_idx, pic.qp, pic.prm, h, gen == Gen::G4)) return rc;
            if (gen == Gen::G4) { /* zero with per-slice offsets (sl_args_g4); _g4 generation only: the _sl kernels do not read the pair */
                h.tc_off = tc_off;
                h.beta_off = beta_off;
            }
            return launch_h265(ctx, h, sl, gen, sb, c_idx, pic.cf, HEVCDBK_KERNEL_AUTO, s);
        },
        [&] {
            return hip_ok(ctx, gen == Gen::G4 ? dbk_launch_sao_g4(sa, sb, s, nx) : dbk_launch_sao(sa, sb, s, nx), "SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
        });
}

/* HEVCDBK_FUSED_ON where the fused kernel does not apply is refused before the device is bound -- by the original entries after
 * (first generation: they looked inside deblock_sao_plane_h265) */
int bind_or_refuse(hevcdbk_context *ctx, const Picture &pic, bool refuse)
{
    if (refuse && !pic.first_gen) return HEVCDBK_ERR_UNSUPPORTED;
    if (int rc = bind(ctx)) return rc;
    return refuse ? HEVCDBK_ERR_UNSUPPORTED : HEVCDBK_OK;
}

/* the SAO pass entries.  first_gen: hevc_sao_filter_device (one ctb_log2); g4_entry: the entry takes a g4 plane */
int sao_pass(hevcdbk_context *ctx, const hevcdbk_device_planes *p, const hevcdbk_sao_plane_cf &sao, const hevcdbk_sao_borders *borders,
             bool first_gen, bool g4_entry, void *hip_stream)
{
    if (!ctx) return HEVCDBK_ERR_ARG;
    const bool g4 = g4_entry && p && g4_kind(p->plane_w, p->plane_h) == 1;
    DbkSaoArgs a;
    if (int rc = first_gen ? sao_args(p, sao.params, sao.params_stride, sao.params_frame_stride, sao.ctb_log2_w, sao.keep, sao.keep_stride,
                                      sao.keep_frame_stride, a)
                           : sao_args_cf(p, sao.params, sao.params_stride, sao.params_frame_stride, sao.ctb_log2_w, sao.ctb_log2_h, sao.keep,
                                         sao.keep_stride, sao.keep_frame_stride, a, g4))
        return rc;
    DbkSaoNox nx, *nxp = nullptr; /* no operand: the kernels without it */
    if (borders) {
        if (int rc = nox_args(borders, a, nx)) return rc;
        nxp = &nx;
    }
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (int rc = sao_square_params(ctx, &a, &sao.ctb_log2_h, 1, s, nxp)) return rc;
    const int rc = hip_ok(ctx, g4 ? dbk_launch_sao_g4(a, (int)p->sample_bytes, s, nxp) : dbk_launch_sao(a, (int)p->sample_bytes, s, nxp), "SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    if (sao.ctb_log2_h != sao.ctb_log2_w)
        if (int rc2 = sao_done(ctx, s, rc != HEVCDBK_OK)) return rc ? rc : rc2; /* the parameter launch is fenced whatever followed it */
    return rc;
}

/* the one-plane deblocking + SAO entries (pic.g4: the entry takes a g4 plane) */
int deblock_sao_one(hevcdbk_context *ctx, Picture pic, const hevcdbk_device_planes *p, int c_idx, const hevcdbk_sao_plane_cf &sao, void *hip_stream)
{
    if (!ctx || bad_fused(pic.fused)) return HEVCDBK_ERR_ARG;
    pic.g4 = pic.g4 && p && g4_kind(p->plane_w, p->plane_h) == 1;
    DbkH265Args h;
    DbkSaoArgs sa;
    DbkSaoNox nx, *nxp = pic.borders ? &nx : nullptr;
    DbkSlOffs sl;
    if (int rc = plane_operands(pic, p, c_idx, sao, h, sa, nx, sl)) return rc;
    if (int rc = bind_or_refuse(ctx, pic, pic.fused == HEVCDBK_FUSED_ON && !fused_can(h, sa, p, c_idx))) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (int rc = sao_square_params(ctx, &sa, &sao.ctb_log2_h, 1, s, nxp)) return rc;
    const int rc = deblock_sao_plane_h265(ctx, pic, p, c_idx, h, sa, sl, nxp, s);
    if (sao.ctb_log2_h != sao.ctb_log2_w)
        if (int rc2 = sao_done(ctx, s, rc != HEVCDBK_OK)) return rc ? rc : rc2; /* the parameter launch is fenced whatever followed it */
    return rc;
}

/* the Y + Cb + Cr entries: deblocking + SAO of all planes in ONE launch where the fused kernel takes every plane, else plane by plane;
 * every plane is checked before the first launch (pic.g4: the entry takes g4 planes) */
int deblock_sao_planes(hevcdbk_context *ctx, Picture pic, const hevcdbk_device_planes *planes, unsigned n_planes, const hevcdbk_sao_plane_cf *sao,
                       void *hip_stream)
{
    const int cf = pic.cf;
    if (!ctx || !planes || !sao || n_planes == 0 || n_planes > 3 || cf < HEVCDBK_CHROMA_400 || cf > HEVCDBK_CHROMA_444 || bad_fused(pic.fused))
        return HEVCDBK_ERR_ARG;
    if (cf == HEVCDBK_CHROMA_400 && n_planes > 1) return HEVCDBK_ERR_ARG;
    bool any_g4 = false, square = true;
    for (unsigned i = 0; i < n_planes; i++) {
        any_g4 = any_g4 || g4_kind(planes[i].plane_w, planes[i].plane_h) == 1;
        square = square && sao[i].ctb_log2_w == sao[i].ctb_log2_h;
    }
    pic.g4 = pic.g4 && any_g4;
    /* 4:2:0 with square CTBs and no operand of a later generation: exactly the original entry, its order of checks included */
    pic.first_gen = pic.first_gen || (cf == HEVCDBK_CHROMA_420 && square && !pic.borders && !pic.so && !pic.g4);
    DbkH265Args h[3];
    DbkSaoArgs sa[3];
    DbkSaoNox nx[3], *nxp = pic.borders ? nx : nullptr; /* ONE operand for the picture: every plane's CTB grid is the luma grid sub-sampled */
    DbkSlOffs sl[3];                                      /* likewise: every plane looks its CTBs up on the luma grid */
    bool can[3] = {false, false, false}, rect = false, all_can = true;
    unsigned log2_h[3] = {0, 0, 0};
    bool one = n_planes >= 2 && pic.fused != HEVCDBK_FUSED_OFF && !planes[0].is_chroma;
    for (unsigned i = 0; i < n_planes; i++) {
        if (int rc = plane_operands(pic, &planes[i], (int)i, sao[i], h[i], sa[i], nx[i], sl[i])) return rc; /* c_idx = plane index: 0 Y, 1 Cb, 2 Cr */
        if (planes[i].n_frames != planes[0].n_frames) return HEVCDBK_ERR_ARG;
        /* chroma planes in the format's geometry of the luma plane: with a g4 plane always; else when planes[0] is the luma plane
         * and the format is not 4:2:0 (as the _nox generation wrote it, 4:2:0 being the original entry's) */
        if (i > 0 && (pic.g4 || (!planes[0].is_chroma && cf != HEVCDBK_CHROMA_420)) &&
            (planes[i].plane_w * sub_w(cf) != planes[0].plane_w || planes[i].plane_h * sub_h(cf) != planes[0].plane_h))
            return HEVCDBK_ERR_ARG;
        log2_h[i] = sao[i].ctb_log2_h;
        rect = rect || sao[i].ctb_log2_h != sao[i].ctb_log2_w;
        can[i] = fused_can(h[i], sa[i], &planes[i], (int)i);
        all_can = all_can && can[i];
        /* one launch: one sample width and depth, one kind of QP, and one luma picture behind all planes (the kernel takes ONE
         * per-slice operand; without it every n_bytes is 0) */
        one = one && (i == 0 || planes[i].is_chroma) && planes[i].sample_bytes == planes[0].sample_bytes &&
              planes[i].bit_depth == planes[0].bit_depth && (h[i].base.qp_map != nullptr) == (h[0].base.qp_map != nullptr) && can[i] &&
              sl[i].n_bytes == sl[0].n_bytes;
    }
    if (int rc = bind_or_refuse(ctx, pic, !one && pic.fused == HEVCDBK_FUSED_ON && !all_can)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (int rc = sao_square_params(ctx, sa, log2_h, n_planes, s, nxp)) return rc;
    int rc = HEVCDBK_OK;
    if (one) {
        const int n = (int)n_planes, sb = (int)planes[0].sample_bytes;
        const hipError_t e = pic.first_gen ? dbk_launch_deblock_sao_multi_h265(h, sa, n, sb, s)
                             : pic.g4     ? dbk_launch_deblock_sao_multi_h265_g4(h, sa, sl[0], n, sb, cf, s, nxp)
                             : pic.so     ? dbk_launch_deblock_sao_multi_h265_sl(h, sa, sl[0], n, sb, cf, s, nxp)
                                          : dbk_launch_deblock_sao_multi_h265_cf(h, sa, n, sb, cf, s, nxp);
        if (!hip_ok(ctx, e, "fused deblocking + SAO launch")) rc = HEVCDBK_ERR_HIP;
    }
    for (unsigned i = 0; !one && i < n_planes && rc == HEVCDBK_OK; i++) /* each plane the kernels of its own generation */
        rc = deblock_sao_plane_h265(ctx, pic, &planes[i], (int)i, h[i], sa[i], sl[i], nxp ? &nxp[i] : nullptr, s);
    if (rect)
        if (int rc2 = sao_done(ctx, s, rc != HEVCDBK_OK)) return rc ? rc : rc2; /* the parameter launch is fenced whatever followed it */
    return rc;
}

} /* namespace */

int hevc_sao_filter_device(hevcdbk_context *ctx, const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params,
                           unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep,
                           unsigned keep_stride, size_t keep_frame_stride, void *hip_stream)
{
    return sao_pass(ctx, p, {params, params_stride, params_frame_stride, ctb_log2, ctb_log2, keep, keep_stride, keep_frame_stride}, nullptr, true,
                    false, hip_stream);
}

int hevcdbk_sao_filter_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params,
                              unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h,
                              const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, void *hip_stream)
{
    return sao_pass(ctx, p, {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, nullptr,
                    false, false, hip_stream);
}

int hevcdbk_sao_filter_device_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params,
                                  unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h,
                                  const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                                  const hevcdbk_sao_borders *borders, void *hip_stream)
{
    return sao_pass(ctx, p, {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, borders,
                    false, false, hip_stream);
}

int hevcdbk_sao_filter_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *p, const hevcdbk_sao_ctb *params,
                                 unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h,
                                 const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                                 const hevcdbk_sao_borders *borders, void *hip_stream)
{
    return sao_pass(ctx, p, {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, borders,
                    false, true, hip_stream);
}

int hevcdbk_h265_sao_borders_device(hevcdbk_context *ctx, const uint16_t *slice_idx, const uint8_t *slice_across, const uint16_t *tile_idx,
                                    int loop_filter_across_tiles_enabled_flag, unsigned ctbs_x, unsigned ctbs_y, unsigned in_stride,
                                    uint8_t *nox, unsigned nox_stride, void *hip_stream)
{
    if (!ctx || !slice_idx || !slice_across || !nox) return HEVCDBK_ERR_ARG;
    if (ctbs_x == 0 || ctbs_y == 0 || ctbs_x > 65535 || ctbs_y > 65535 || in_stride < ctbs_x || nox_stride < ctbs_x) return HEVCDBK_ERR_ARG;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const hipError_t e = dbk_launch_sao_borders(slice_idx, slice_across, tile_idx, loop_filter_across_tiles_enabled_flag != 0, (int)ctbs_x,
                                                (int)ctbs_y, (int)in_stride, nox, (int)nox_stride, s);
    return hip_ok(ctx, e, "SAO border derivation launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* ---- deblocking followed by SAO in one call ---------------------------------------------- */

int hevc_deblock_sao_device(hevcdbk_context *ctx, const hevcdbk_device_planes *p, unsigned qp, const hevcdbk_tables *tables,
                            const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2,
                            const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, int fused, void *hip_stream)
{
    if (!ctx || (fused != HEVCDBK_FUSED_AUTO && fused != HEVCDBK_FUSED_OFF && fused != HEVCDBK_FUSED_ON)) return HEVCDBK_ERR_ARG;
    DbkSaoArgs sa;
    if (int rc = sao_args(p, params, params_stride, params_frame_stride, ctb_log2, keep, keep_stride, keep_frame_stride, sa)) return rc;
    DbkArgs da;
    if (int rc = planes_to_args(p, qp, tables, da)) return rc;
    if (int rc = bind(ctx)) return rc;
    return deblock_sao_plane(ctx, p, qp, tables, da, sa, fused, hip_stream ? (hipStream_t)hip_stream : ctx->compute);
}

/* ---- spec-exact deblocking + SAO of one plane: the original 4:2:0 entry, chroma formats (_cf), SAO borders (_nox), per-slice
 * offsets (_sl), planes sized in multiples of 4 (_g4: the chroma planes of 1920x1080 are 960x540) -- one body, deblock_sao_one ---- */

int hevc_deblock_sao_h265_device(hevcdbk_context *ctx, const hevcdbk_device_planes *p, int c_idx, unsigned qp,
                                 const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                 size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride,
                                 size_t keep_frame_stride, int fused, void *hip_stream)
{
    return deblock_sao_one(ctx, {HEVCDBK_CHROMA_420, qp, prm, fused, nullptr, nullptr, true, false}, p, c_idx,
                           {params, params_stride, params_frame_stride, ctb_log2, ctb_log2, keep, keep_stride, keep_frame_stride}, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *p, int c_idx, int chroma_format_idc, unsigned qp,
                                    const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                    size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep,
                                    unsigned keep_stride, size_t keep_frame_stride, int fused, void *hip_stream)
{
    return deblock_sao_one(ctx, {chroma_format_idc, qp, prm, fused, nullptr, nullptr, false, false}, p, c_idx,
                           {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *p, int c_idx, int chroma_format_idc, unsigned qp,
                                        const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                        size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep,
                                        unsigned keep_stride, size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                        void *hip_stream)
{
    return deblock_sao_one(ctx, {chroma_format_idc, qp, prm, fused, borders, nullptr, false, false}, p, c_idx,
                           {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *p, int c_idx, int chroma_format_idc, unsigned qp,
                                       const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                       size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep,
                                       unsigned keep_stride, size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                       const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    return deblock_sao_one(ctx, {chroma_format_idc, qp, prm, fused, borders, slice_offsets, false, false}, p, c_idx,
                           {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *p, int c_idx, int chroma_format_idc, unsigned qp,
                                       const hevcdbk_h265_params *prm, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                       size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep,
                                       unsigned keep_stride, size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                       const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    return deblock_sao_one(ctx, {chroma_format_idc, qp, prm, fused, borders, slice_offsets, false, true}, p, c_idx,
                           {params, params_stride, params_frame_stride, ctb_log2_w, ctb_log2_h, keep, keep_stride, keep_frame_stride}, hip_stream);
}

/* ---- Y, U, V of a batch: deblocking + SAO of all planes in ONE launch where the fused kernel takes every plane ---- */

int hevc_deblock_sao_device_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes, unsigned qp,
                                   const hevcdbk_tables *tables, const hevcdbk_sao_plane *sao, int fused, void *hip_stream)
{
    if (!ctx || !planes || !sao || n_planes == 0 || n_planes > 3 ||
        (fused != HEVCDBK_FUSED_AUTO && fused != HEVCDBK_FUSED_OFF && fused != HEVCDBK_FUSED_ON))
        return HEVCDBK_ERR_ARG;
    DbkArgs da[3];
    DbkSaoArgs sa[3];
    bool one = n_planes >= 2 && fused != HEVCDBK_FUSED_OFF && !planes[0].is_chroma;
    for (unsigned i = 0; i < n_planes; i++) {
        if (int rc = sao_args(&planes[i], sao[i].params, sao[i].params_stride, sao[i].params_frame_stride, sao[i].ctb_log2, sao[i].keep,
                              sao[i].keep_stride, sao[i].keep_frame_stride, sa[i]))
            return rc;
        if (int rc = planes_to_args(&planes[i], qp, tables, da[i])) return rc;
        if (planes[i].n_frames != planes[0].n_frames) return HEVCDBK_ERR_ARG;
        one = one && (i == 0 || planes[i].is_chroma) && planes[i].sample_bytes == planes[0].sample_bytes &&
              planes[i].bit_depth == planes[0].bit_depth && (da[i].qp_map != nullptr) == (da[0].qp_map != nullptr) &&
              dbk_deblock_sao_supports(da[i], sa[i], (int)planes[i].sample_bytes, planes[i].is_chroma != 0);
    }
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    if (one)
        return hip_ok(ctx, dbk_launch_deblock_sao_multi(da, sa, (int)n_planes, (int)planes[0].sample_bytes, s), "fused deblocking + SAO launch")
                   ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
    /* plane by plane; every plane is checked before the first launch */
    if (fused == HEVCDBK_FUSED_ON)
        for (unsigned i = 0; i < n_planes; i++)
            if (!dbk_deblock_sao_supports(da[i], sa[i], (int)planes[i].sample_bytes, planes[i].is_chroma != 0)) return HEVCDBK_ERR_UNSUPPORTED;
    for (unsigned i = 0; i < n_planes; i++)
        if (int rc = deblock_sao_plane(ctx, &planes[i], qp, tables, da[i], sa[i], fused, s)) return rc;
    return HEVCDBK_OK;
}

/* the spec-exact generations of the same: one body, deblock_sao_planes */
int hevc_deblock_sao_h265_device_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes, unsigned qp,
                                        const hevcdbk_h265_params *prm, const hevcdbk_sao_plane *sao, int fused, void *hip_stream)
{
    hevcdbk_sao_plane_cf cf[3];
    for (unsigned i = 0; sao && i < n_planes && i < 3; i++)
        cf[i] = {sao[i].params, sao[i].params_stride, sao[i].params_frame_stride, sao[i].ctb_log2, sao[i].ctb_log2, sao[i].keep, sao[i].keep_stride,
                 sao[i].keep_frame_stride};
    return deblock_sao_planes(ctx, {HEVCDBK_CHROMA_420, qp, prm, fused, nullptr, nullptr, true, false}, planes, n_planes, sao ? cf : nullptr, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_planes_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                           int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *prm,
                                           const hevcdbk_sao_plane_cf *sao, int fused, void *hip_stream)
{
    return deblock_sao_planes(ctx, {chroma_format_idc, qp, prm, fused, nullptr, nullptr, false, false}, planes, n_planes, sao, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_planes_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                               int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *prm,
                                               const hevcdbk_sao_plane_cf *sao, int fused, const hevcdbk_sao_borders *borders,
                                               void *hip_stream)
{
    return deblock_sao_planes(ctx, {chroma_format_idc, qp, prm, fused, borders, nullptr, false, false}, planes, n_planes, sao, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_planes_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                              int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *prm,
                                              const hevcdbk_sao_plane_cf *sao, int fused, const hevcdbk_sao_borders *borders,
                                              const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    return deblock_sao_planes(ctx, {chroma_format_idc, qp, prm, fused, borders, slice_offsets, false, false}, planes, n_planes, sao, hip_stream);
}

int hevcdbk_h265_deblock_sao_device_planes_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                              int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *prm,
                                              const hevcdbk_sao_plane_cf *sao, int fused, const hevcdbk_sao_borders *borders,
                                              const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    return deblock_sao_planes(ctx, {chroma_format_idc, qp, prm, fused, borders, slice_offsets, false, true}, planes, n_planes, sao, hip_stream);
}

/* ---- per-slice deblocking offsets (H.265 8.7.2.5.3 / 8.7.2.5.5: the pair of the slice that holds q0,0): the operand from the decoder's arrays ---- */

int hevcdbk_h265_slice_offsets_device(hevcdbk_context *ctx, const uint16_t *slice_idx, unsigned in_stride, const int8_t *slice_table,
                                      unsigned n_slices, unsigned ctbs_x, unsigned ctbs_y, int8_t *offs, unsigned offs_stride,
                                      void *hip_stream)
{
    if (!ctx || !slice_idx || !offs || (uintptr_t)offs % 2 != 0 || (n_slices != 0 && !slice_table)) return HEVCDBK_ERR_ARG;
    if (ctbs_x == 0 || ctbs_y == 0 || ctbs_x > 65535 || ctbs_y > 65535 || (unsigned long long)ctbs_x * ctbs_y > (1ull << 30) || /* one lane per CTB, numbered in an int */
        in_stride < ctbs_x || offs_stride < ctbs_x)
        return HEVCDBK_ERR_ARG;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const hipError_t e = dbk_launch_h265_slice_offsets(slice_idx, (int)in_stride, slice_table, n_slices, (int)ctbs_x, (int)ctbs_y, offs,
                                                       (int)offs_stride, s);
    return hip_ok(ctx, e, "slice offset derivation launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

/* ---- semi-planar chroma: one plane of interleaved Cb / Cr pairs (the _sp entry) ---------------------------------------------- */

int hevcdbk_h265_filter_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp, const hevcdbk_h265_params *params,
                                  int kernel_variant, const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    if (!ctx || !planes) return HEVCDBK_ERR_ARG;
    if (int rc = sp_plane_ok(planes)) return rc;
    DbkH265Args h;
    if (int rc = h265_args(planes, 1, qp, params, h, true)) return rc; /* h.c_qp_offset = cb_qp_offset: the even samples */
    const int cr_qp_offset = params ? params->cr_qp_offset : 0;
    DbkSlOffs sl;
    if (int rc = sl_args_g4(slice_offsets, planes, 1, HEVCDBK_CHROMA_420, h, sl)) return rc;
    int variant = kernel_variant, map_override;
    if (int rc = check_variant(variant, map_override, false)) return rc;
    if (map_override == 2) return HEVCDBK_ERR_UNSUPPORTED; /* HEVCDBK_MAP_LINEAR: the packed kernels have the row map only */
    const bool pack = dbk_packed_h265_sp_supports(h, (int)planes->sample_bytes);
    if (variant == HEVCDBK_KERNEL_PACKED && !pack) return HEVCDBK_ERR_UNSUPPORTED;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const hipError_t e = (variant != HEVCDBK_KERNEL_GENERIC && pack) ? dbk_launch_packed_h265_sp(h, sl, cr_qp_offset, (int)planes->sample_bytes, s)
                                                                    : dbk_launch_h265_sp(h, sl, cr_qp_offset, (int)planes->sample_bytes, s);
    return hip_ok(ctx, e, "kernel launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

int hevcdbk_sao_filter_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params_cb,
                                 const hevcdbk_sao_ctb *params_cr, unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2,
                                 const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, const hevcdbk_sao_borders *borders,
                                 void *hip_stream)
{
    if (!ctx || !planes) return HEVCDBK_ERR_ARG;
    DbkSaoArgs a;
    DbkSaoNox nx;
    if (int rc = sp_sao_args(planes, params_cb, params_cr, params_stride, params_frame_stride, ctb_log2, keep, keep_stride, keep_frame_stride,
                             borders, a, nx))
        return rc;
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const hipError_t e = dbk_launch_sao_sp(a, reinterpret_cast<const DbkSaoCtb *>(params_cr), (int)planes->sample_bytes, s, borders ? &nx : nullptr);
    return hip_ok(ctx, e, "SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
}

int hevcdbk_h265_deblock_sao_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp, const hevcdbk_h265_params *prm,
                                       const hevcdbk_sao_ctb *params_cb, const hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                                       size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride,
                                       size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                       const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream)
{
    if (!ctx || !planes || bad_fused(fused)) return HEVCDBK_ERR_ARG;
    DbkSaoArgs sa;
    DbkSaoNox nx;
    if (int rc = sp_sao_args(planes, params_cb, params_cr, params_stride, params_frame_stride, ctb_log2, keep, keep_stride, keep_frame_stride,
                             borders, sa, nx))
        return rc;
    DbkH265Args h;
    if (int rc = h265_args(planes, 1, qp, prm, h, true)) return rc;
    DbkSlOffs sl;
    if (int rc = sl_args_g4(slice_offsets, planes, 1, HEVCDBK_CHROMA_420, h, sl)) return rc;
    if (fused == HEVCDBK_FUSED_ON) return HEVCDBK_ERR_UNSUPPORTED; /* no fused kernel for this layout: before any launch */
    if (int rc = bind(ctx)) return rc;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : ctx->compute;
    const int sb = (int)planes->sample_bytes, cr_qp_offset = prm ? prm->cr_qp_offset : 0;
    const int tc_off = h.tc_off, beta_off = h.beta_off; /* zero with per-slice offsets (sl_args_g4) */
    /* the two launches through the context's scratch plane, as deblock_sao_plane_h265 runs them for a g4 plane */
    return through_scratch(
        ctx, planes, s, sa,
        [&](const hevcdbk_device_planes &first) {
            if (int rc = h265_args(&first, 1, qp, prm, h, true)) return rc;
            h.tc_off = tc_off;
            h.beta_off = beta_off;
            const hipError_t e = dbk_packed_h265_sp_supports(h, sb) ? dbk_launch_packed_h265_sp(h, sl, cr_qp_offset, sb, s)
                                                                    : dbk_launch_h265_sp(h, sl, cr_qp_offset, sb, s);
            return hip_ok(ctx, e, "kernel launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
        },
        [&] {
            const hipError_t e = dbk_launch_sao_sp(sa, reinterpret_cast<const DbkSaoCtb *>(params_cr), sb, s, borders ? &nx : nullptr);
            return hip_ok(ctx, e, "SAO launch") ? HEVCDBK_OK : HEVCDBK_ERR_HIP;
        });
}

} /* extern "C" */
