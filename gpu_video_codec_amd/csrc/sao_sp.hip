/*
 * sao_sp.hip -- gfx950 kernels of sample adaptive offset (H.265 8.7.3) for a semi-planar chroma plane (hevcdbk_sao_filter_device_sp and
 * the SAO stage of hevcdbk_h265_deblock_sao_device_sp; sao_sp.h): one plane of interleaved Cb / Cr pairs, both components in one
 * launch, each with its own CTB entries.  plane_w x plane_h, the CTB grid, the keep map and the boundary bytes are those of ONE
 * component; a row of the plane holds 2 * plane_w samples.
 *
 * One lane owns one 8x8 block of sample PAIRS (the keep map's unit, inside one CTB), a wave 64 x 64 pairs, a workgroup a strip of
 * 256 x 64: the geometry of sao.hip, so a row of 8 lanes of the 8-bit kernel is one 128-byte line.  A lane fetches both components'
 * CTB entries, the keep byte and the boundary byte once; saonox::block_mask is computed once and serves both components (the two
 * samples of a pair have one position).  Three kinds of wave:
 *   - the ballot over the masks is zero (nearly every wave): the packed block procedures, BORDER = 0, on buffer resources with the
 *     row in the scalar offset;
 *   - a block of 4 columns or 4 rows in the wave (the last column / row of blocks of a plane whose size is a multiple of 4, not 8):
 *     the per-sample procedure with a component stride of 2 (saosp::block_px) for the whole wave;
 *   - every other wave on a picture border or a slice / tile boundary: the packed procedures, BORDER = 2, with the mask; rows outside
 *     the picture are read as the nearest row inside, halo pairs outside a row as a dword inside it -- the mask discards what comes
 *     of them.
 * Every row leaves as ONE 16-byte store (two for 16-bit containers) holding both components.
 */
#include <hip/hip_runtime.h>

#include "deblock_kernels.h"
#include "launch_select.h"
#include "sao_sp.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

/* workgroup -> (256 x 64 strip, frame): the renumbered 1-D grid of sao.hip (each XCD works through a contiguous range of strips), or
 * the plain 3-D numbering for grids too large for the exact reciprocal divisions */
template <bool SWZ>
__device__ __forceinline__ bool sp_strip(const DbkFusedGrid &g, int &wx, int &wy, int &f)
{
    if constexpr (!SWZ) {
        wx = blockIdx.x; wy = blockIdx.y; f = blockIdx.z;
        return true;
    } else {
        const uint32_t id = blockIdx.x;
        const uint32_t logical = (id & 7u) * g.per_xcd + (id >> 3);
        if (logical >= g.total) return false; /* padding workgroup */
        const uint32_t fr = g.tiles_per_frame == 1u ? logical : __umulhi(logical, g.magic_tpf);
        const uint32_t in_frame = logical - fr * g.tiles_per_frame;
        const uint32_t row = g.tiles_x == 1u ? in_frame : __umulhi(in_frame, g.magic_tx);
        wx = (int)(in_frame - row * g.tiles_x); wy = (int)row; f = (int)fr;
        return true;
    }
}

/* what a lane knows of its block before it touches a sample */
struct SpLane {
    int x, y0, f;
    DbkSaoCtb c0, c1; /* the even samples' entry, the odd samples' */
    bool kept;
    uint32_t nox, m;  /* the CTB's boundary byte, the block's mask */
};

template <bool SWZ>
__device__ __forceinline__ bool sp_lane(const DbkSaoArgs &a, const DbkSaoCtb *params_cr, const DbkFusedGrid &g, const DbkSaoNox &nx, SpLane &L)
{
    int wx, wy;
    if (!sp_strip<SWZ>(g, wx, wy, L.f)) return false;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    L.x = (wx * 4 + wv) * 64 + (l & 7) * 8;
    L.y0 = wy * 64 + (l >> 3) * 8;
    if (L.x >= a.plane_w || L.y0 >= a.plane_h) return false;
    L.nox = nx.nox ? saonox::ctb_byte(nx, L.f, L.x, L.y0, a.ctb_log2) : 0u; /* no bytes: nothing forbidden */
    const long long at = (long long)L.f * a.params_frame_stride + (long long)(L.y0 >> a.ctb_log2) * a.params_stride + (L.x >> a.ctb_log2);
    L.c0 = a.params[at];
    L.c1 = params_cr[at];
    L.kept = a.keep && a.keep[(long long)L.f * a.keep_frame_stride + (long long)(L.y0 >> 3) * a.keep_stride + (L.x >> 3)];
    L.m = saonox::block_mask<8>(L.nox, L.x, L.y0, a.plane_w, a.plane_h, a.ctb_log2); /* the picture border included */
    return true;
}

__device__ __forceinline__ saosp::Plane sp_plane(const DbkSaoArgs &a, int f)
{
    return saosp::Plane{a.src + (long long)f * a.frame_stride, a.dst + (long long)f * a.frame_stride, a.pitch, a.plane_w, a.plane_h,
                        a.ctb_log2, a.max_v, a.band_shift};
}

/* a 16-byte store with a scalar row offset is followed by two wait states before anything may write its data registers
 * (profiles/r04/store_hazard.md; sao_kernel_body.inc and deblock_sp.hip do the same) */
__device__ __forceinline__ void sp_store128(const u32x4 w, __amdgpu_buffer_rsrc_t rd, uint32_t voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b128(w, rd, voff, soff, 0);
    asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory");
}

/* a wave of whole blocks.  SB = bytes per sample: a lane's row piece is 16 * SB bytes at byte 16 * SB * (x / 8) of the row */
template <int SB, int BORDER>
__device__ __forceinline__ void sp_packed_wave(const DbkSaoArgs &a, const SpLane &L)
{
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h; /* < 2^31: checked by the launcher */
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.src) + (long long)L.f * a.frame_stride, 0,
                                                                        plane_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(a.dst + (long long)L.f * a.frame_stride, 0, plane_bytes, 0x00020000);
    const int sp = __builtin_amdgcn_readfirstlane((int)a.pitch);
    const uint32_t bx = (uint32_t)L.x * 2u * SB;
    const uint32_t vrow = (uint32_t)L.y0 * (uint32_t)a.pitch + bx;
    const uint32_t vup = vrow - (uint32_t)a.pitch; /* raw row 0 = image row y0 - 1; BORDER 0: y0 >= 8 */
    /* (vector offset, scalar offset) of raw row j: off the border the lane's offset once and the row in the scalar offset; on it the
     * row number clamped into the picture */
    auto at = [&](int j, uint32_t &vo, int &so) {
        if constexpr (BORDER == 0) {
            vo = vup;
            so = j * sp;
        } else {
            const int y = L.y0 - 1 + j;
            vo = (uint32_t)(y < 0 ? 0 : (y >= a.plane_h ? a.plane_h - 1 : y)) * (uint32_t)a.pitch + bx;
            so = 0;
        }
    };
    /* the halo pairs: the dword in front of the piece and the one behind it; outside the row (BORDER 2 only) a dword inside it */
    auto halos = [&](uint32_t vo, int so, uint32_t &hl, uint32_t &hr) {
        uint32_t lo = vo - 4u, ro = vo + 16u * SB;
        if constexpr (BORDER != 0) {
            if (L.x == 0) lo = vo;
            if (L.x + 8 >= a.plane_w) ro = vo + 16u * SB - 4u;
        }
        hl = __builtin_amdgcn_raw_buffer_load_b32(rs, lo, so, 0);
        hr = __builtin_amdgcn_raw_buffer_load_b32(rs, ro, so, 0);
    };
    if constexpr (SB == 1) {
        auto load = [&](int j, uint32_t (&d)[4], uint32_t &hl, uint32_t &hr, bool halo) {
            uint32_t vo;
            int so;
            at(j, vo, so);
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            if (halo) halos(vo, so, hl, hr);
        };
        auto store = [&](int r, const uint32_t (&d)[4]) {
            u32x4 w;
            w.x = d[0]; w.y = d[1]; w.z = d[2]; w.w = d[3];
            if constexpr (BORDER == 0) sp_store128(w, rd, vrow, r * sp);
            else sp_store128(w, rd, vrow + (uint32_t)r * (uint32_t)a.pitch, 0);
        };
        saosp::block8<BORDER>(load, store, L.x, L.y0, a.plane_w, a.plane_h, L.c0, L.c1, L.kept, L.m);
    } else {
        auto load = [&](int j, uint32_t (&d)[8], uint32_t &hl, uint32_t &hr, bool halo) {
            uint32_t vo;
            int so;
            at(j, vo, so);
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so, 0);
            const u32x4 u = __builtin_amdgcn_raw_buffer_load_b128(rs, vo + 16u, so, 0);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            d[4] = u.x; d[5] = u.y; d[6] = u.z; d[7] = u.w;
            if (halo) halos(vo, so, hl, hr);
        };
        auto store = [&](int r, const uint32_t (&d)[8]) {
            u32x4 w, v;
            w.x = d[0]; w.y = d[1]; w.z = d[2]; w.w = d[3];
            v.x = d[4]; v.y = d[5]; v.z = d[6]; v.w = d[7];
            const uint32_t vo = BORDER == 0 ? vrow : vrow + (uint32_t)r * (uint32_t)a.pitch;
            const int so = BORDER == 0 ? r * sp : 0;
            sp_store128(w, rd, vo, so);
            sp_store128(v, rd, vo + 16u, so);
        };
        saosp::block16<BORDER>(load, store, L.x, L.y0, a.plane_w, a.plane_h, L.c0, L.c1, L.kept, a.max_v, a.band_shift, L.m);
    }
}

template <typename T, int SB, bool SWZ>
__device__ __forceinline__ void sp_packed_body(const DbkSaoArgs &a, const DbkSaoCtb *params_cr, const DbkFusedGrid &g, const DbkSaoNox &nx)
{
    SpLane L;
    if (!sp_lane<SWZ>(a, params_cr, g, nx, L)) return;
    if (__builtin_amdgcn_ballot_w64(L.m != 0u) == 0ull) {
        sp_packed_wave<SB, 0>(a, L);
        return;
    }
    if (__builtin_amdgcn_ballot_w64(L.x + 8 > a.plane_w || L.y0 + 8 > a.plane_h) != 0ull) {
        saosp::block_px<T>(sp_plane(a, L.f), L.nox, L.x, L.y0, L.c0, L.c1, L.kept);
        return;
    }
    sp_packed_wave<SB, 2>(a, L);
}

/* 8-bit samples */
template <bool SWZ>
__global__ __launch_bounds__(256) void sao8_sp_kernel(const DbkSaoArgs a, const DbkSaoCtb *params_cr, const DbkFusedGrid g, const DbkSaoNox nx)
{
    sp_packed_body<uint8_t, 1, SWZ>(a, params_cr, g, nx);
}

/* 16-bit containers up to 12 bit */
template <bool SWZ>
__global__ __launch_bounds__(256) void sao16_sp_kernel(const DbkSaoArgs a, const DbkSaoCtb *params_cr, const DbkFusedGrid g, const DbkSaoNox nx)
{
    sp_packed_body<uint16_t, 2, SWZ>(a, params_cr, g, nx);
}

/* every depth, planes aligned to one 4-sample word: the per-sample procedure in every lane */
template <typename T, bool SWZ>
__global__ __launch_bounds__(256) void sao_sp_kernel(const DbkSaoArgs a, const DbkSaoCtb *params_cr, const DbkFusedGrid g, const DbkSaoNox nx)
{
    SpLane L;
    if (!sp_lane<SWZ>(a, params_cr, g, nx, L)) return;
    saosp::block_px<T>(sp_plane(a, L.f), L.nox, L.x, L.y0, L.c0, L.c1, L.kept);
}

} /* namespace */

bool dbk_sao_sp_packed_supports(const DbkSaoArgs &a, int sample_bytes)
{
    const unsigned long long piece = sample_bytes == 1 ? 16 : 32; /* a lane's row piece */
    if (a.pitch % piece != 0 || a.frame_stride % piece != 0 || (uintptr_t)a.src % piece != 0 || (uintptr_t)a.dst % piece != 0) return false;
    if ((unsigned long long)a.pitch * (unsigned long long)a.plane_h >= (1ull << 31)) return false; /* 32-bit buffer offsets */
    if (sample_bytes == 1) return a.max_v == 255 && a.band_shift == 3;
    return a.max_v <= 4095 && a.band_shift >= 3 && (1 << (a.band_shift + 5)) - 1 == a.max_v; /* the packed procedure's int16 fields */
}

hipError_t dbk_launch_sao_sp(const DbkSaoArgs &a, const DbkSaoCtb *params_cr, int sample_bytes, hipStream_t stream, const DbkSaoNox *nxp)
{
    using namespace dbksel;
    if (nothing_to_do(a)) return hipSuccess;
    const SaoGrid sg = sao_grid(a);
    const DbkSaoNox nx = nxp ? *nxp : DbkSaoNox{nullptr, 0, 0};
    const bool packed = dbk_sao_sp_packed_supports(a, sample_bytes);
    with_bool(sg.swz, [&](auto SWZ) {
        if (sample_bytes == 1 && packed) hipLaunchKernelGGL(sao8_sp_kernel<SWZ>, sg.grid, sg.block, 0, stream, a, params_cr, sg.g, nx);
        else if (sample_bytes == 1) hipLaunchKernelGGL((sao_sp_kernel<uint8_t, SWZ>), sg.grid, sg.block, 0, stream, a, params_cr, sg.g, nx);
        else if (packed) hipLaunchKernelGGL(sao16_sp_kernel<SWZ>, sg.grid, sg.block, 0, stream, a, params_cr, sg.g, nx);
        else hipLaunchKernelGGL((sao_sp_kernel<uint16_t, SWZ>), sg.grid, sg.block, 0, stream, a, params_cr, sg.g, nx);
    });
    return hipGetLastError();
}
