/*
 * deblock_sp.hip -- gfx950 kernels of the spec-exact mode for a semi-planar chroma plane (hevcdbk_h265_filter_device_sp of the C
 * ABI; deblock_sp.h): one plane of interleaved Cb / Cr pairs, both components in one launch.
 *
 * One lane owns one offset 8x8 block of sample PAIRS.  Cb and Cr of a 4:2:0 picture share the bS arrays, the QP map and the
 * per-slice offset pairs, so a lane fetches those once and filters two blocks with them; only cQpPicOffset -- and through it tC --
 * differs between the two.  Built on the most general form there is, like the _g4 kernels (deblock_g4.hip): a per-lane qPL (one QP
 * or a map is a wave-uniform test), per-slice pairs from an array that has no bytes when the call has none (every load reads 0
 * through the buffer range check) with the launch's own pair added, and the geometry of planes that are multiples of 4: "this half
 * is inside" is 8 bx < plane_w, 8 by < plane_h (deblock_h265.h g4_right_in / g4_below_in).  plane_w / plane_h, nbx / nby and the bS
 * layouts are those of ONE component; a row of the plane holds 2 * plane_w samples.
 *
 * The packed kernels: a block row of 8-bit pairs is 16 bytes at byte offset 16 bx - 8, of 16-bit pairs 32 bytes at 32 bx - 16.
 * Interior waves fetch their eight rows with dwordx4 accesses and a scalar row offset; frame-edge waves address the two halves of a
 * row separately and push a half or a row that lies outside the picture out of the buffer's range (the load returns 0, the store is
 * dropped): no lane masks.  The arithmetic is the planar kernels' chroma procedure (deblock_packed_h265.h, deblock_packed16.h),
 * called once per component between deblock_sp.h's split and merge.  One workgroup per block row (the row map only).
 */
#include <hip/hip_runtime.h>

#include "deblock_h265_quad4.h"
#include "deblock_packed16.h"
#include "deblock_sp.h"
#include "deblock_sp_dev.h"
#include "launch_select.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kOob = 0xfffffff0u; /* voffset >= num_records: load returns 0, store is dropped */

/* ---- 32-bit arithmetic, every operand kind: samples of any depth, planes aligned to one 4-sample word ---- */
template <typename T>
__global__ __launch_bounds__(256) void dbk_h265_sp_kernel(const DbkH265Args h, const DbkSlOffs sl, const int cr_qp_offset)
{
    using Q = Quad4<T>;
    using W = typename Q::W;
    const DbkArgs &a = h.base;
    const int bx = blockIdx.x * 64 + threadIdx.x;
    const int by = blockIdx.y * 4 + threadIdx.y;
    const int f = blockIdx.z;
    if (bx >= a.nbx || by >= a.nby) return;

    int entry[4], qpl[4], tc_off[4], beta_off[4];
    dbk::sp_block_operands(h, sl, f, bx, by, entry, qpl, tc_off, beta_off);
    /* chroma ignores bS 1 (8.7.2.5): blocks with nothing to filter move no samples at all when filtering in place */
    bool any = false;
#pragma unroll
    for (int s = 0; s < 4; s++) any |= (entry[s] & dbk::kH265BsMask) == 2;
    if (!any && a.src == a.dst) return;

    const uint8_t *src = a.src + (long long)f * a.frame_stride;
    uint8_t *dst = a.dst + (long long)f * a.frame_stride;
    const int x0 = bx * 8 - 4, y0 = by * 8 - 4;
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, a.plane_w);

    int v[2][8][8]; /* [component][row][column] */
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        const uint8_t *row = src + (long long)y * a.pitch + (long long)x0 * 2 * (int)sizeof(T);
#pragma unroll
        for (int j = 0; j < 4; j++) { /* word j = the pairs 2j, 2j + 1 of the block's row */
            W w = Q::zero();
            if (rowv && (j < 2 ? lv : rv)) w = *reinterpret_cast<const W *>(row + 4 * j * sizeof(T));
            Q::unpack(w, v[0][r][2 * j], v[1][r][2 * j], v[0][r][2 * j + 1], v[1][r][2 * j + 1]);
        }
    }

    if (any) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const dbk::H265Prm prm = {0, 0, c ? cr_qp_offset : h.c_qp_offset, a.shift, a.max_v};
            dbk::filter_block_h265_sl<1>(v[c], entry, qpl, prm, tc_off, beta_off);
        }
    }

#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool rowv = (unsigned)y < (unsigned)a.plane_h;
        uint8_t *row = dst + (long long)y * a.pitch + (long long)x0 * 2 * (int)sizeof(T);
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (rowv && (j < 2 ? lv : rv))
                *reinterpret_cast<W *>(row + 4 * j * sizeof(T)) = Q::pack(v[0][r][2 * j], v[1][r][2 * j], v[0][r][2 * j + 1], v[1][r][2 * j + 1]);
    }
}

/* ---- packed-int16 arithmetic ---- */

/* a 16-byte store with a scalar row offset is followed by two wait states before anything may write its data registers
 * (profiles/r04/store_hazard.md; the 16-bit fused kernel's stores do the same) */
__device__ __forceinline__ void sp_store128(const u32x4 w, __amdgpu_buffer_rsrc_t rd, uint32_t voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b128(w, rd, voff, soff, 0);
    asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory");
}

/* 8-bit samples.  EDGE false: an interior wave (by scalar, all eight rows and both halves of every lane inside the picture) */
template <bool EDGE>
__device__ __forceinline__ void sp8_body(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int f, int by, int bx)
{
    const DbkArgs &a = h.base;
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, a.plane_w);
    const int y0 = by * 8 - 4;
    const uint32_t xoff = (uint32_t)(bx * 16 - 8);
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(a.dst + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);

    uint32_t D[8][4];
    if constexpr (!EDGE) {
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, xoff, (y0 + r) * (int)a.pitch, 0);
            D[r][0] = w.x; D[r][1] = w.y; D[r][2] = w.z; D[r][3] = w.w;
        }
    } else {
        const uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
        const uint32_t lbits = lv ? 0u : kOob, rbits = rv ? 0u : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob; /* scalar */
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            const u32x2 l = __builtin_amdgcn_raw_buffer_load_b64(rs, off | lbits | ob, 0, 0);
            const u32x2 rr = __builtin_amdgcn_raw_buffer_load_b64(rs, (off + 8u) | rbits | ob, 0, 0);
            D[r][0] = l.x; D[r][1] = l.y; D[r][2] = rr.x; D[r][3] = rr.y;
        }
    }

    dbk::H265Seg sb, sr;
    dbk::sp_seg_params(h, sl, cr_qp_offset, f, bx, by, 0, 255, sb, sr);

    uint32_t Lb[8], Rb[8], Lr[8], Rr[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        dbk::sp_split8<0>(D[r], Lb[r], Rb[r]);
        dbk::sp_split8<1>(D[r], Lr[r], Rr[r]);
    }
    dbk::packed_filter_block_h265<true>(Lb, Rb, sb);
    dbk::packed_filter_block_h265<true>(Lr, Rr, sr);
#pragma unroll
    for (int r = 0; r < 8; r++) dbk::sp_merge8(Lb[r], Rb[r], Lr[r], Rr[r], D[r]);

    if constexpr (!EDGE) {
        int spitch = __builtin_amdgcn_readfirstlane((int)a.pitch);
        asm volatile("" : "+s"(spitch)); /* the row offsets are built again, not carried across the filter (packed_body) */
#pragma unroll
        for (int r = 0; r < 8; r++) {
            u32x4 w;
            w.x = D[r][0]; w.y = D[r][1]; w.z = D[r][2]; w.w = D[r][3];
            sp_store128(w, rd, xoff, (y0 + r) * spitch);
        }
    } else {
        uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
        asm volatile("" : "+v"(base));
        const uint32_t lbits = lv ? 0u : kOob, rbits = rv ? 0u : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob;
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            u32x2 l, rr;
            l.x = D[r][0]; l.y = D[r][1]; rr.x = D[r][2]; rr.y = D[r][3];
            __builtin_amdgcn_raw_buffer_store_b64(l, rd, off | lbits | ob, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b64(rr, rd, (off + 8u) | rbits | ob, 0, 0);
        }
    }
}

/* 16-bit containers up to 12 bit: a row of the block is two 16-byte halves */
template <bool EDGE>
__device__ __forceinline__ void sp16_body(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int f, int by, int bx)
{
    const DbkArgs &a = h.base;
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, a.plane_w);
    const int y0 = by * 8 - 4;
    const uint32_t xoff = (uint32_t)(bx * 32 - 16);
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(a.dst + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);

    uint32_t D[8][8];
    const uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
    const uint32_t lbits = lv ? 0u : kOob, rbits = rv ? 0u : kOob;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        u32x4 l, rr;
        if constexpr (!EDGE) {
            l = __builtin_amdgcn_raw_buffer_load_b128(rs, xoff, (y0 + r) * (int)a.pitch, 0);
            rr = __builtin_amdgcn_raw_buffer_load_b128(rs, xoff + 16u, (y0 + r) * (int)a.pitch, 0);
        } else {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob;
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            l = __builtin_amdgcn_raw_buffer_load_b128(rs, off | lbits | ob, 0, 0);
            rr = __builtin_amdgcn_raw_buffer_load_b128(rs, (off + 16u) | rbits | ob, 0, 0);
        }
        D[r][0] = l.x; D[r][1] = l.y; D[r][2] = l.z; D[r][3] = l.w;
        D[r][4] = rr.x; D[r][5] = rr.y; D[r][6] = rr.z; D[r][7] = rr.w;
    }

    dbk::H265Seg sb, sr;
    dbk::sp_seg_params(h, sl, cr_qp_offset, f, bx, by, a.shift, a.max_v, sb, sr);

    uint32_t Wb[8][4], Wr[8][4];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        dbk::sp_split16<0>(D[r], Wb[r]);
        dbk::sp_split16<1>(D[r], Wr[r]);
    }
    dbk::packed_filter_block16_h265<true>(Wb, sb, a.max_v);
    dbk::packed_filter_block16_h265<true>(Wr, sr, a.max_v);
#pragma unroll
    for (int r = 0; r < 8; r++) dbk::sp_merge16(Wb[r], Wr[r], D[r]);

    int spitch = __builtin_amdgcn_readfirstlane((int)a.pitch);
    asm volatile("" : "+s"(spitch));
    uint32_t base2 = (uint32_t)(y0 * spitch) + xoff;
    asm volatile("" : "+v"(base2));
#pragma unroll
    for (int r = 0; r < 8; r++) {
        u32x4 l, rr;
        l.x = D[r][0]; l.y = D[r][1]; l.z = D[r][2]; l.w = D[r][3];
        rr.x = D[r][4]; rr.y = D[r][5]; rr.z = D[r][6]; rr.w = D[r][7];
        if constexpr (!EDGE) {
            sp_store128(l, rd, xoff, (y0 + r) * spitch);
            sp_store128(rr, rd, xoff + 16u, (y0 + r) * spitch);
        } else {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob;
            const uint32_t off = base2 + (uint32_t)r * (uint32_t)spitch;
            sp_store128(l, rd, off | lbits | ob, 0);
            sp_store128(rr, rd, (off + 16u) | rbits | ob, 0);
        }
    }
}

/* one workgroup = one block row of one frame (blockIdx.x = by, .y = frame), one lane = one block; a wave whose last lane has its
 * right half inside the picture -- then so has every lane, and every lane owns a block -- and which does not hold bx == 0 is an
 * interior wave when the block row's eight sample rows are inside as well */
__device__ __forceinline__ bool sp_wave(const DbkArgs &a, int &by, int &f, int &bx, bool &interior)
{
    by = blockIdx.x;
    f = blockIdx.y;
    bx = threadIdx.x;
    const int wave_bx0 = __builtin_amdgcn_readfirstlane(bx) & ~63;
    interior = wave_bx0 > 0 && dbk::g4_right_in(wave_bx0 + 63, a.plane_w) && by > 0 && dbk::g4_below_in(by, a.plane_h);
    return bx < a.nbx; /* idle lanes leave at once: there is no barrier in these kernels */
}

__global__ __launch_bounds__(1024) void dbk_packed_h265_sp_kernel(const DbkH265Args h, const DbkSlOffs sl, const int cr_qp_offset)
{
    int by, f, bx;
    bool interior;
    if (!sp_wave(h.base, by, f, bx, interior)) return;
    if (interior) sp8_body<false>(h, sl, cr_qp_offset, f, by, bx);
    else sp8_body<true>(h, sl, cr_qp_offset, f, by, bx);
}

__global__ __launch_bounds__(1024) void dbk_packed16_h265_sp_kernel(const DbkH265Args h, const DbkSlOffs sl, const int cr_qp_offset)
{
    int by, f, bx;
    bool interior;
    if (!sp_wave(h.base, by, f, bx, interior)) return;
    if (interior) sp16_body<false>(h, sl, cr_qp_offset, f, by, bx);
    else sp16_body<true>(h, sl, cr_qp_offset, f, by, bx);
}

} /* namespace */

hipError_t dbk_launch_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int sample_bytes, hipStream_t stream)
{
    using namespace dbksel;
    if (nothing_to_do(h.base)) return hipSuccess;
    with_int<1, 2>(sample_bytes, [&](auto SB) {
        hipLaunchKernelGGL(dbk_h265_sp_kernel<sample_t<SB>>, generic_grid(h.base), generic_block(), 0, stream, h, sl, cr_qp_offset);
    });
    return hipGetLastError();
}

bool dbk_packed_h265_sp_supports(const DbkH265Args &h, int sample_bytes)
{
    const DbkArgs &a = h.base;
    if ((unsigned long long)a.pitch * (unsigned long long)a.plane_h >= (1ull << 31)) return false; /* 32-bit buffer offsets */
    if (a.nbx > 1024) return false;                                                                /* one workgroup per block row */
    const unsigned long long al = sample_bytes == 1 ? 8 : 16;                                      /* one half of a block's row */
    if (a.pitch % al != 0 || a.frame_stride % al != 0 || (uintptr_t)a.src % al != 0 || (uintptr_t)a.dst % al != 0) return false;
    return sample_bytes == 1 ? a.max_v == 255 : a.max_v <= 4095; /* chroma: 5 * max_v + 4 fits int16 up to 12 bit (deblock_packed16.h) */
}

hipError_t dbk_launch_packed_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int sample_bytes, hipStream_t stream)
{
    if (dbksel::nothing_to_do(h.base)) return hipSuccess;
    if (!dbk_packed_h265_sp_supports(h, sample_bytes)) return hipErrorInvalidValue;
    const dim3 block((unsigned)((h.base.nbx + 63) / 64 * 64), 1, 1);
    const dim3 grid((unsigned)h.base.nby, (unsigned)h.base.n_frames, 1);
    if (sample_bytes == 1) hipLaunchKernelGGL(dbk_packed_h265_sp_kernel, grid, block, 0, stream, h, sl, cr_qp_offset);
    else hipLaunchKernelGGL(dbk_packed16_h265_sp_kernel, grid, block, 0, stream, h, sl, cr_qp_offset);
    return hipGetLastError();
}
