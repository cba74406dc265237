/*
 * deblock_sl.hip -- gfx950 kernels of the spec-exact mode with per-slice deblocking offsets (deblock_sl.h; hevcdbk_h265_slice_offsets
 * of the C ABI): the 32-bit block filter of every operand kind, and the producer of the operand.
 *
 * The operand is a kernel argument of its own (DbkSlOffs beside DbkH265Args) and the kernels that take it have names of their own,
 * in a translation unit of their own: every kernel without the operand keeps its argument layout and its machine code.
 *
 * Same mapping as deblock_h265.hip: one lane owns one offset 8x8 block, a wave owns 64 consecutive blocks of a block row.  What is
 * new per lane is three 16-bit loads -- the pairs of the CTBs that hold q0,0 of its segments (above-right, below-left, below-right
 * of the block centre) -- through a buffer resource whose range is the array itself, with 24-bit multiply-adds for the offsets,
 * issued together with the bS loads ahead of the first wait.
 */
#include <hip/hip_runtime.h>

#include "deblock_h265_quad4.h"
#include "deblock_sl_dev.h"
#include "launch_select.h"

namespace {

/* CF 0 = luma, 1..3 = a chroma plane of a picture of that chroma_format_idc; one QP (base.qp_map == NULL) or a QP map */
template <typename T, int CF>
__global__ __launch_bounds__(256) void dbk_h265_sl_kernel(const DbkH265Args h, const DbkSlOffs sl)
{
    using Q = Quad4<T>;
    using W = typename Q::W;
    constexpr int sx = CF == 0 ? 1 : dbk::ChromaFmt<CF == 0 ? 1 : CF>::sx, sy = CF == 0 ? 1 : dbk::ChromaFmt<CF == 0 ? 1 : CF>::sy;
    const DbkArgs &a = h.base;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (bx >= a.nbx || by >= a.nby) return;

    int entry[4];
    dbk::load_block_bs_h265(a.vert_bs + (long long)f * a.vert_bs_stride, a.hor_bs + (long long)f * a.hor_bs_stride, bx, by,
                            a.nbx, a.nby, a.vstride, a.hstride, entry);
    unsigned ar, bl, br;
    dbk_sl_load_pairs<sx, sy>(sl, f, bx, by, a.plane_w * sx, a.plane_h * sy, ar, bl, br);
    /* chroma ignores bS 1 (8.7.2.5): blocks with nothing to filter move no samples at all when filtering in place */
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; s++) any |= CF != 0 ? (entry[s] & dbk::kH265BsMask) == 2 : (entry[s] & dbk::kH265BsMask) != 0;
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
        int qpl[4], tc_off[4], beta_off[4];
        dbk::h265_block_qpl_xy(a.qp_map ? a.qp_map + (long long)f * a.map_frame_stride : nullptr, a.map_stride, a.ctu_log2, sx, sy,
                               a.plane_w * sx, a.plane_h * sy, x0, y0, h.qp, qpl);
        dbk::h265_sl_seg_offs(ar, bl, br, tc_off, beta_off);
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

/* the producer: one lane per CTB, the pair of the CTB's slice out of the slice table (beta, tc), (0, 0) for a slice index the
 * table does not hold; one 2-byte store per CTB */
__global__ __launch_bounds__(256) void dbk_h265_slice_offsets_kernel(const uint16_t *slice_idx, int in_stride, const int8_t *table,
                                                                     unsigned n_slices, int ctbs_x, int ctbs_y, int8_t *offs,
                                                                     int offs_stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ctbs_x * ctbs_y) return;
    const int cy = i / ctbs_x, cx = i - cy * ctbs_x;
    const unsigned s = slice_idx[(long long)cy * in_stride + cx];
    char2 p = make_char2(0, 0);
    if (s < n_slices) p = make_char2(table[2 * s], table[2 * s + 1]);
    *reinterpret_cast<char2 *>(offs + 2 * ((long long)cy * offs_stride + cx)) = p;
}

} /* namespace */

hipError_t dbk_launch_h265_sl(const DbkH265Args &h, const DbkSlOffs &sl, int sample_bytes, int chroma_format, hipStream_t stream)
{
    using namespace dbksel;
    if (chroma_format != 0 && !chroma_format_ok(chroma_format)) return hipErrorInvalidValue; /* 0 = luma */
    if (nothing_to_do(h.base)) return hipSuccess;
    with_int<1, 2>(sample_bytes, [&](auto SB) {
        with_int<0, 1, 2, 3>(chroma_format, [&](auto CF) {
            hipLaunchKernelGGL((dbk_h265_sl_kernel<sample_t<SB>, CF>), generic_grid(h.base), generic_block(), 0, stream, h, sl);
        });
    });
    return hipGetLastError();
}

hipError_t dbk_launch_h265_slice_offsets(const uint16_t *slice_idx, int in_stride, const int8_t *table, unsigned n_slices, int ctbs_x,
                                         int ctbs_y, int8_t *offs, int offs_stride, hipStream_t stream)
{
    const unsigned total = (unsigned)ctbs_x * (unsigned)ctbs_y; /* <= 2^30: the entry point checks */
    if (ctbs_x <= 0 || ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(dbk_h265_slice_offsets_kernel, dim3((total + 255u) / 256u), dim3(256), 0, stream, slice_idx, in_stride,
                       table, n_slices, ctbs_x, ctbs_y, offs, offs_stride);
    return hipGetLastError();
}
