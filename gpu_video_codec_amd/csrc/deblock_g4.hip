/*
 * deblock_g4.hip -- gfx950 kernel of the spec-exact mode for chroma planes whose width and height are multiples of 4, not 8 (the
 * _g4 entries of the C ABI; deblock_h265.h load_block_bs_h265_g4): the 32-bit block filter of every operand kind.
 *
 * Built on the most general form there is, the per-slice-offset kernel of deblock_sl.hip: one lane owns one offset 8x8 block, three
 * 16-bit loads fetch the pairs of the CTBs that hold q0,0 of its segments.  A call without the operand hands in an array of no
 * bytes (sl.n_bytes == 0: every load reads 0 through the buffer range check and never memory) and its own pair in h.tc_off /
 * h.beta_off, which the kernel adds; a call with the operand hands in zeros there.  The new geometry is an argument of nobody
 * else: every other kernel keeps its argument layout and its machine code.
 *
 * What changes against deblock_sl.hip is the meaning of two comparisons: the right half of a block is inside the picture when
 * 8 bx < plane_w (not bx < nbx - 1), and the same test decides whether x = 8 bx is an edge; likewise for rows.
 */
#include <hip/hip_runtime.h>

#include "deblock_h265_quad4.h"
#include "deblock_sl_dev.h"
#include "launch_select.h"

namespace {

/* CF 1..3 = a chroma plane of a picture of that chroma_format_idc; one QP (base.qp_map == NULL) or a QP map */
template <typename T, int CF>
__global__ __launch_bounds__(256) void dbk_h265_g4_kernel(const DbkH265Args h, const DbkSlOffs sl)
{
    using Q = Quad4<T>;
    using W = typename Q::W;
    constexpr int sx = dbk::ChromaFmt<CF>::sx, sy = dbk::ChromaFmt<CF>::sy;
    const DbkArgs &a = h.base;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (bx >= a.nbx || by >= a.nby) return;

    int entry[4];
    dbk::load_block_bs_h265_g4(a.vert_bs + (long long)f * a.vert_bs_stride, a.hor_bs + (long long)f * a.hor_bs_stride, bx, by,
                               a.plane_w, a.plane_h, a.vstride, a.hstride, entry);
    unsigned ar, bl, br;
    dbk_sl_load_pairs<sx, sy>(sl, f, bx, by, a.plane_w * sx, a.plane_h * sy, ar, bl, br);
    /* chroma ignores bS 1 (8.7.2.5): blocks with nothing to filter move no samples at all when filtering in place */
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; s++) any |= (entry[s] & dbk::kH265BsMask) == 2;
    if (!any && a.src == a.dst) return;

    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    const int x0 = bx * 8 - 4, y0 = by * 8 - 4;
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, a.plane_w);

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
        int qpl[4], tc_off[4], beta_off[4];
        dbk::h265_block_qpl_xy(a.qp_map ? a.qp_map + (long long)f * a.map_frame_stride : nullptr, a.map_stride, a.ctu_log2, sx, sy,
                               a.plane_w * sx, a.plane_h * sy, x0, y0, h.qp, qpl);
        dbk::h265_sl_seg_offs(ar, bl, br, tc_off, beta_off);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            tc_off[s] += h.tc_off;
            beta_off[s] += h.beta_off;
        }
        const dbk::H265Prm prm = {0, 0, h.c_qp_offset, a.shift, a.max_v};
        dbk::filter_block_h265_sl<CF>(v, entry, qpl, prm, tc_off, beta_off);
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

} /* namespace */

hipError_t dbk_launch_h265_g4(const DbkH265Args &h, const DbkSlOffs &sl, int sample_bytes, int chroma_format, hipStream_t stream)
{
    using namespace dbksel;
    if (!chroma_format_ok(chroma_format)) return hipErrorInvalidValue;
    if (nothing_to_do(h.base)) return hipSuccess;
    with_int<1, 2>(sample_bytes, [&](auto SB) {
        with_int<1, 2, 3>(chroma_format, [&](auto CF) {
            hipLaunchKernelGGL((dbk_h265_g4_kernel<sample_t<SB>, CF>), generic_grid(h.base), generic_block(), 0, stream, h, sl);
        });
    });
    return hipGetLastError();
}
