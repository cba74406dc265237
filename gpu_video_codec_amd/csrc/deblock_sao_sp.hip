/*
 * deblock_sao_sp.hip -- gfx950 kernels of deblocking + SAO in ONE kernel for a semi-planar chroma plane (hevcdbk_h265_deblock_sao_device_sp_fused
 * of the C ABI): one plane of interleaved Cb / Cr pairs, spec-exact mode, 8-bit samples and 16-bit containers up to 12 bit.  The body
 * is deblock_sao_sp_fused.h; the kernel of a whole frame (Y plane + pair plane) is in deblock_kernels.hip, beside the luma body.
 */
#include <hip/hip_runtime.h>

#include "deblock_sao_sp_fused.h"
#include "launch_select.h"

namespace {

constexpr int kThreads = 256; /* four waves: 221 (8-bit) / 153 (16-bit) stage-1 lanes, four stage-2 waves */

__global__ __launch_bounds__(kThreads) void dbk_sao_fused_h265_sp_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl,
                                                                         const DbkSaoCtb *params_cr, const int cr_qp_offset)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    spf::body<1, kThreads>(fa.d, fa.s, fa.g, params_cr, cr_qp_offset, nx, sl, fused_tile, blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void dbk_sao_fused16_h265_sp_kernel(const DbkFusedH265Args fa, const DbkSaoNox nx, const DbkSlOffs sl,
                                                                           const DbkSaoCtb *params_cr, const int cr_qp_offset)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t fused_tile[];
    spf::body<2, kThreads>(fa.d, fa.s, fa.g, params_cr, cr_qp_offset, nx, sl, fused_tile, blockIdx.x);
}

template <int SB>
unsigned long long tiles_of(int plane_w, int plane_h, unsigned long long &tx)
{
    typedef spf::Geo<SB> G;
    tx = (unsigned long long)((plane_w + G::kTileW - 1) / G::kTileW);
    return tx * (unsigned long long)((plane_h + G::kTileH - 1) / G::kTileH);
}

} /* namespace */

/* the guards of the fused pair-plane kernels, stated once: the one-plane launcher, the frame launcher and the host entries ask here */
bool dbk_deblock_sao_sp_supports(const DbkH265Args &h, const DbkSaoArgs &s, int sample_bytes)
{
    const DbkArgs &d = h.base;
    if (d.by_count != 0 || d.max_v != s.max_v) return false;
    if (sample_bytes == 1) {
        if (d.max_v != 255 || s.band_shift != 3) return false;
    } else { /* 16-bit containers up to 12 bit: chroma's 5 * max_v + 4 fits int16 (deblock_packed16.h), SAO's int16 fields (sao_packed.h) */
        if (sample_bytes != 2 || d.max_v > 4095 || s.band_shift < 3 || (1 << (s.band_shift + 5)) - 1 != s.max_v) return false;
    }
    if (d.plane_w != s.plane_w || d.plane_h != s.plane_h || d.n_frames != s.n_frames || d.n_frames > 65535) return false;
    if (d.plane_w < 8 || d.plane_h < 8 || d.plane_w % 4 != 0 || d.plane_h % 4 != 0) return false;
    /* a lane's row piece: 16 bytes of 8-bit pairs, 32 bytes of 16-bit ones */
    const unsigned long long piece = 16ull * (unsigned)sample_bytes;
    if (d.pitch != s.pitch || d.frame_stride != s.frame_stride || d.pitch % piece != 0 || d.frame_stride % piece != 0 ||
        (uintptr_t)d.src % piece != 0 || (uintptr_t)s.dst % piece != 0)
        return false;
    if ((unsigned long long)d.pitch * (unsigned long long)d.plane_h >= (1ull << 31)) return false; /* 32-bit buffer offsets */
    unsigned long long tx;
    const unsigned long long tiles = sample_bytes == 1 ? tiles_of<1>(d.plane_w, d.plane_h, tx) : tiles_of<2>(d.plane_w, d.plane_h, tx);
    return tiles * (unsigned long long)d.n_frames + 8 < (1ull << 31) && tiles * tiles < (1ull << 32) &&
           (tiles * d.n_frames + 8) * tiles < (1ull << 32); /* exact reciprocal divisions: dividend < 2^32 / divisor (dbk_deblock_sao_supports) */
}

/* 1-D grid of the pair plane's tiles, a multiple of 8 workgroups */
unsigned dbk_deblock_sao_sp_grid(int plane_w, int plane_h, int n_frames, int sample_bytes, DbkFusedGrid &g)
{
    const int tw = sample_bytes == 1 ? spf::Geo<1>::kTileW : spf::Geo<2>::kTileW, th = sample_bytes == 1 ? spf::Geo<1>::kTileH : spf::Geo<2>::kTileH;
    const dbksel::RenumberedGrid r = dbksel::renumbered_grid((plane_w + tw - 1) / tw, (plane_h + th - 1) / th, n_frames);
    g = r.g;
    return r.wgs;
}

hipError_t dbk_launch_deblock_sao_h265_sp(const DbkH265Args &h, const DbkSaoArgs &s, const DbkSaoCtb *params_cr, const DbkSlOffs &sl,
                                          int cr_qp_offset, int sample_bytes, hipStream_t stream, const DbkSaoNox *nxp)
{
    if (dbksel::nothing_to_do(h.base)) return hipSuccess;
    if (!dbk_deblock_sao_sp_supports(h, s, sample_bytes)) return hipErrorInvalidValue;
    DbkFusedH265Args fa;
    fa.d = h;
    fa.s = s;
    const dim3 grid(dbk_deblock_sao_sp_grid(h.base.plane_w, h.base.plane_h, h.base.n_frames, sample_bytes, fa.g), 1, 1);
    const DbkSaoNox nx = nxp ? *nxp : DbkSaoNox{nullptr, 0, 0}; /* no bytes: no direction is forbidden */
    if (sample_bytes == 1)
        hipLaunchKernelGGL(dbk_sao_fused_h265_sp_kernel, grid, dim3(kThreads), spf::Geo<1>::kLds, stream, fa, nx, sl, params_cr, cr_qp_offset);
    else
        hipLaunchKernelGGL(dbk_sao_fused16_h265_sp_kernel, grid, dim3(kThreads), spf::Geo<2>::kLds, stream, fa, nx, sl, params_cr, cr_qp_offset);
    return hipGetLastError();
}
