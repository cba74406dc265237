/*
 * deblock_h265.hip -- gfx950 kernels of the spec-exact mode (ITU-T H.265 clause 8.7.2):
 * the block filter, the bS derivation (8.7.2.4) and the 4:2:0 chroma bS gather.
 *
 * Same mapping as the reference-exact kernels: one lane owns one offset 8x8 block, a wave owns 64 consecutive blocks
 * of a block row, rows outside the picture are never loaded or stored.  Arithmetic is the 32-bit form of
 * deblock_h265.h for every operand kind (8/16-bit samples, luma/chroma, scalar QP or QP map).
 */
#include <hip/hip_runtime.h>

#include "deblock_h265.h"
#include "deblock_h265_quad4.h"
#include "deblock_kernels.h"
#include "launch_select.h"

namespace {

template <typename T, bool CHROMA>
__global__ __launch_bounds__(256) void dbk_h265_kernel(const DbkH265Args h)
{
    using Q = Quad4<T>;
    using W = typename Q::W;
    const DbkArgs &a = h.base;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (bx >= a.nbx || by >= a.nby) return;

    int entry[4];
    dbk::load_block_bs_h265(a.vert_bs + (long long)f * a.vert_bs_stride, a.hor_bs + (long long)f * a.hor_bs_stride, bx, by,
                            a.nbx, a.nby, a.vstride, a.hstride, entry);
    /* chroma ignores bS 1 (8.7.2.5): blocks with nothing to filter move no samples at all when filtering in place */
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; s++) any |= CHROMA ? (entry[s] & dbk::kH265BsMask) == 2 : (entry[s] & dbk::kH265BsMask) != 0;
    if (!any && a.src == a.dst) return;

    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    const int x0 = bx * 8 - 4, y0 = by * 8 - 4;
    const bool lv = bx > 0, rv = bx < a.nbx - 1;

    int v[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        const uint8_t *row = src + (long long)y * a.pitch + (long long)x0 * (int)sizeof(T);
        W l = Q::zero(), rr = Q::zero();
        if (rowv && lv) l = *reinterpret_cast<const W *>(row);
        if (rowv && rv) rr = *reinterpret_cast<const W *>(row + 4 * sizeof(T));
        Q::unpack(l, v[r][0], v[r][1], v[r][2], v[r][3]);
        Q::unpack(rr, v[r][4], v[r][5], v[r][6], v[r][7]);
    }

    if (any) {
        int qpl[4];
        const int sc = CHROMA ? 2 : 1;
        dbk::h265_block_qpl(a.qp_map ? a.qp_map + (long long)f * a.map_frame_stride : nullptr, a.map_stride, a.ctu_log2, sc,
                            a.plane_w * sc, a.plane_h * sc, x0, y0, h.qp, qpl);
        const dbk::H265Prm prm = {h.tc_off, h.beta_off, h.c_qp_offset, a.shift, a.max_v};
        dbk::filter_block_h265<CHROMA>(v, entry, qpl, prm);
    }

#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        uint8_t *row = dst + (long long)y * a.pitch + (long long)x0 * (int)sizeof(T);
        if (rowv && lv) *reinterpret_cast<W *>(row) = Q::pack(v[r][0], v[r][1], v[r][2], v[r][3]);
        if (rowv && rv) *reinterpret_cast<W *>(row + 4 * sizeof(T)) = Q::pack(v[r][4], v[r][5], v[r][6], v[r][7]);
    }
}

/* chroma planes of 4:2:2 (CF 2) and 4:4:4 (CF 3) pictures: dbk_h265_kernel<T, true> with the format's QP-map scaling per axis and
 * its QpC rule (deblock_h265.h ChromaFmt, h265_chroma_qp_cf) -- a kernel of its own, so that the 4:2:0 instantiations above keep
 * their machine code */
template <typename T, int CF>
__global__ __launch_bounds__(256) void dbk_h265_cf_kernel(const DbkH265Args h)
{
    using Q = Quad4<T>;
    using W = typename Q::W;
    const DbkArgs &a = h.base;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (bx >= a.nbx || by >= a.nby) return;

    int entry[4];
    dbk::load_block_bs_h265(a.vert_bs + (long long)f * a.vert_bs_stride, a.hor_bs + (long long)f * a.hor_bs_stride, bx, by,
                            a.nbx, a.nby, a.vstride, a.hstride, entry);
    /* chroma ignores bS 1 (8.7.2.5): blocks with nothing to filter move no samples at all when filtering in place */
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; s++) any |= (entry[s] & dbk::kH265BsMask) == 2;
    if (!any && a.src == a.dst) return;

    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    const int x0 = bx * 8 - 4, y0 = by * 8 - 4;
    const bool lv = bx > 0, rv = bx < a.nbx - 1;

    int v[8][8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        const uint8_t *row = src + (long long)y * a.pitch + (long long)x0 * (int)sizeof(T);
        W l = Q::zero(), rr = Q::zero();
        if (rowv && lv) l = *reinterpret_cast<const W *>(row);
        if (rowv && rv) rr = *reinterpret_cast<const W *>(row + 4 * sizeof(T));
        Q::unpack(l, v[r][0], v[r][1], v[r][2], v[r][3]);
        Q::unpack(rr, v[r][4], v[r][5], v[r][6], v[r][7]);
    }

    if (any) {
        int qpl[4];
        constexpr int sx = dbk::ChromaFmt<CF>::sx, sy = dbk::ChromaFmt<CF>::sy;
        dbk::h265_block_qpl_xy(a.qp_map ? a.qp_map + (long long)f * a.map_frame_stride : nullptr, a.map_stride, a.ctu_log2, sx, sy,
                               a.plane_w * sx, a.plane_h * sy, x0, y0, h.qp, qpl);
        const dbk::H265Prm prm = {h.tc_off, h.beta_off, h.c_qp_offset, a.shift, a.max_v};
        dbk::filter_block_h265_chroma_cf<CF>(v, entry, qpl, prm);
    }

#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        uint8_t *row = dst + (long long)y * a.pitch + (long long)x0 * (int)sizeof(T);
        if (rowv && lv) *reinterpret_cast<W *>(row) = Q::pack(v[r][0], v[r][1], v[r][2], v[r][3]);
        if (rowv && rv) *reinterpret_cast<W *>(row + 4 * sizeof(T)) = Q::pack(v[r][4], v[r][5], v[r][6], v[r][7]);
    }
}

/* 8.7.2.4: one thread per bS entry; blockIdx.y = 0 vertical edges, 1 horizontal edges */
__global__ __launch_bounds__(256) void dbk_h265_bs_kernel(const dbk::H265Units u, int w, int h, uint8_t *vert, uint8_t *hor)
{
    const long long uw = w / 4;
    const int vstride = w / 8 + 1, hstride = w / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.y == 0) {
        if (i >= (long long)vstride * (h / 4)) return;
        const int y4 = (int)(i / vstride), bx = (int)(i % vstride);
        const bool edge = bx > 0 && bx < w / 8; /* x = 0 and x = w: picture boundary */
        vert[i] = edge ? (uint8_t)dbk::h265_bs_of_edge(u, y4 * uw + 2 * bx - 1, y4 * uw + 2 * bx, true) : (uint8_t)0;
    } else {
        if (i >= (long long)(h / 8 + 1) * hstride) return;
        const int by = (int)(i / hstride), x4 = (int)(i % hstride);
        const bool edge = by > 0 && by < h / 8;
        hor[i] = edge ? (uint8_t)dbk::h265_bs_of_edge(u, (2 * by - 1) * uw + x4, (2 * by) * uw + x4, false) : (uint8_t)0;
    }
}

/* 4:2:0 chroma arrays = the luma entry at twice the chroma position (8.7.2.5: bS[xDk * SubWidthC][yDm * SubHeightC]) */
__global__ __launch_bounds__(256) void dbk_h265_chroma_bs_kernel(const uint8_t *vert, const uint8_t *hor, int w, int h,
                                                                 uint8_t *cvert, uint8_t *chor)
{
    const int cw = w / 2, ch = h / 2;
    const int vstride = w / 8 + 1, hstride = w / 4, cvstride = cw / 8 + 1, chstride = cw / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.y == 0) {
        if (i >= (long long)cvstride * (ch / 4)) return;
        const int m = (int)(i / cvstride), bx = (int)(i % cvstride);
        cvert[i] = vert[(long long)(2 * m) * vstride + 2 * bx];
    } else {
        if (i >= (long long)(ch / 8 + 1) * chstride) return;
        const int by = (int)(i / chstride), m = (int)(i % chstride);
        chor[i] = hor[(long long)(2 * by) * hstride + 2 * m];
    }
}

/* the chroma arrays of a 4:2:2 (SX 2, SY 1) or 4:4:4 (SX 1, SY 1) picture, in the chroma plane's own 4-sample-granular layout:
 * the luma entry at bS[xDk * SubWidthC][yDm * SubHeightC] (8.7.2.5.5), i.e. vertical chroma edge (row m, column bx) = luma
 * (row m * SY, column bx * SX), horizontal chroma edge (row by, column m) = luma (row by * SY, column m * SX) */
template <int SX, int SY>
__global__ __launch_bounds__(256) void dbk_h265_chroma_bs_cf_kernel(const uint8_t *vert, const uint8_t *hor, int w, int h,
                                                                    uint8_t *cvert, uint8_t *chor)
{
    const int cw = w / SX, ch = h / SY;
    const int vstride = w / 8 + 1, hstride = w / 4, cvstride = cw / 8 + 1, chstride = cw / 4;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.y == 0) {
        if (i >= (long long)cvstride * (ch / 4)) return;
        const int m = (int)(i / cvstride), bx = (int)(i % cvstride);
        cvert[i] = vert[(long long)(SY * m) * vstride + SX * bx];
    } else {
        if (i >= (long long)(ch / 8 + 1) * chstride) return;
        const int by = (int)(i / chstride), m = (int)(i % chstride);
        chor[i] = hor[(long long)(SY * by) * hstride + SX * m];
    }
}

} /* namespace */

hipError_t dbk_launch_h265(const DbkH265Args &h, int sample_bytes, bool chroma, hipStream_t stream)
{
    using namespace dbksel;
    if (nothing_to_do(h.base)) return hipSuccess;
    with_int<1, 2>(sample_bytes, [&](auto SB) {
        with_bool(chroma, [&](auto CHROMA) {
            hipLaunchKernelGGL((dbk_h265_kernel<sample_t<SB>, CHROMA>), generic_grid(h.base), generic_block(), 0, stream, h);
        });
    });
    return hipGetLastError();
}

hipError_t dbk_launch_h265_bs(const void *flags, const void *mv0, const void *mv1, const void *ref0, const void *ref1, int w,
                              int h, uint8_t *vert, uint8_t *hor, uint8_t *cvert, uint8_t *chor, hipStream_t stream)
{
    const dbk::H265Units u = {(const uint16_t *)flags, (const int16_t *)mv0, (const int16_t *)mv1, (const int32_t *)ref0,
                              (const int32_t *)ref1};
    const long long nv = (long long)(w / 8 + 1) * (h / 4), nh = (long long)(h / 8 + 1) * (w / 4);
    const long long n = nv > nh ? nv : nh;
    hipLaunchKernelGGL(dbk_h265_bs_kernel, dim3((unsigned)((n + 255) / 256), 2, 1), dim3(256), 0, stream, u, w, h, vert, hor);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !cvert || !chor) return e;
    return dbk_launch_h265_chroma_bs(vert, hor, w, h, cvert, chor, stream);
}

hipError_t dbk_launch_h265_chroma_bs(const uint8_t *vert, const uint8_t *hor, int w, int h, uint8_t *cvert, uint8_t *chor,
                                     hipStream_t stream)
{
    const int cw = w / 2, ch = h / 2;
    const long long nv = (long long)(cw / 8 + 1) * (ch / 4), nh = (long long)(ch / 8 + 1) * (cw / 4);
    const long long n = nv > nh ? nv : nh;
    hipLaunchKernelGGL(dbk_h265_chroma_bs_kernel, dim3((unsigned)((n + 255) / 256), 2, 1), dim3(256), 0, stream, vert, hor, w, h,
                       cvert, chor);
    return hipGetLastError();
}

hipError_t dbk_launch_h265_cf(const DbkH265Args &h, int sample_bytes, int chroma_format, hipStream_t stream)
{
    using namespace dbksel;
    if (chroma_format == 1) return dbk_launch_h265(h, sample_bytes, true, stream);
    if (!chroma_format_ok(chroma_format)) return hipErrorInvalidValue;
    if (nothing_to_do(h.base)) return hipSuccess;
    with_int<1, 2>(sample_bytes, [&](auto SB) {
        with_int<2, 3>(chroma_format, [&](auto CF) {
            hipLaunchKernelGGL((dbk_h265_cf_kernel<sample_t<SB>, CF>), generic_grid(h.base), generic_block(), 0, stream, h);
        });
    });
    return hipGetLastError();
}

hipError_t dbk_launch_h265_chroma_bs_cf(const uint8_t *vert, const uint8_t *hor, int w, int h, int chroma_format, uint8_t *cvert,
                                        uint8_t *chor, hipStream_t stream)
{
    if (chroma_format == 1) return dbk_launch_h265_chroma_bs(vert, hor, w, h, cvert, chor, stream);
    if (!dbksel::chroma_format_ok(chroma_format)) return hipErrorInvalidValue;
    const int cw = chroma_format == 3 ? w : w / 2, ch = h;
    const long long nv = (long long)(cw / 8 + 1) * (ch / 4), nh = (long long)(ch / 8 + 1) * (cw / 4);
    const long long n = nv > nh ? nv : nh;
    const dim3 grid((unsigned)((n + 255) / 256), 2, 1);
    if (chroma_format == 2) hipLaunchKernelGGL((dbk_h265_chroma_bs_cf_kernel<2, 1>), grid, dim3(256), 0, stream, vert, hor, w, h, cvert, chor);
    else hipLaunchKernelGGL((dbk_h265_chroma_bs_cf_kernel<1, 1>), grid, dim3(256), 0, stream, vert, hor, w, h, cvert, chor);
    return hipGetLastError();
}
