/*
 * deblock_sao_sp_fused.h -- deblocking (H.265 8.7.2, spec-exact mode) and sample adaptive offset (8.7.3) of a semi-planar chroma
 * plane -- one plane of interleaved Cb / Cr pairs -- in ONE kernel, the deblocked samples handed from the first stage to the second
 * through the workgroup's LDS tile: the structure of fused_body / fused_body16 (deblock_sao_fused.inc) for the pair layout.  Included
 * by deblock_sao_sp.hip (the kernel of one pair plane) and by deblock_kernels.hip (the kernel of a whole frame: the Y plane's tiles run
 * the luma body, the pair plane's tiles this one).
 *
 * A workgroup owns a tile of kTileW x kTileH PAIRS:
 *   1. one lane per offset 8x8 block of pairs (deblock_sp.hip's lane): the kBlocksX x kBlocksY blocks that cover the tile plus one
 *      sample of halo all round.  The lane loads its eight rows of pairs, fetches the block's operands once for both components
 *      (deblock_sp_dev.h), takes the rows apart (deblock_sp.h), runs the planar chroma block procedure once per component and writes the
 *      two results DE-INTERLEAVED into LDS: a tile row holds the even samples' kComp bytes and behind them the odd samples' kComp
 *      bytes, so the tile is two component-planar tiles side by side in the rows of ONE tile of the planar kernels' size;
 *   2. one workgroup barrier;
 *   3. the tile's 32 x 32 regions are dealt to the waves; a lane takes a block of 8 pairs x 2 rows (4 lanes across, 16 down: with
 *      32-sample CTBs the wave holds one CTB, i.e. one SAO path per component).  Each component's rows come out of its planar tile
 *      exactly as the planar fused kernels read theirs -- no preloaded rows in registers -- and go through the planar block procedures
 *      (sao_packed.h); the first component's two output rows wait (2 or 4 VGPRs per row) for the second's and leave merged
 *      (deblock_sp.h) as 16-byte stores of pairs.
 * Built on the general form the _sp and _g4 kernels use: a per-lane qPL (one QP or a map is a wave-uniform test), per-slice pairs from
 * an array of no bytes when the call has none with the launch's own pair added, sizes that are multiples of 4, boundary bytes that may
 * be absent (nothing forbidden), the keep map.
 *
 *   samples   tile (pairs)   stage-1 lanes           LDS rows x pitch
 *   8-bit     96 x 128       13 x 17 = 221           136 x 208 (2 x 104): byte for byte the 8-bit luma tile and its HBM footprint
 *   16-bit    64 x 128        9 x 17 = 153           136 x 288 (2 x 144): the 16-bit luma tile
 * One lane = one pair-block with both components: half the lanes of "one lane per component", no cross-lane traffic.
 *
 * The per-lane procedures of both stages are DBK_HD, like the headers they are built from: tests/fused_sp_sim drives them on the CPU
 * tile by tile, with a host array standing for the LDS tile.  The loads, the operand fetch and the stores are the device part below.
 */
#pragma once
#include <stdint.h>

#include "deblock_packed.h"
#include "deblock_packed_h265.h"
#include "deblock_packed16.h"
#include "deblock_sp.h"
#include "sao_packed.h"

namespace spf {

template <int SB /* bytes per sample */>
struct Geo {
    static constexpr int kTileW = SB == 1 ? 96 : 64;           /* pairs per tile row */
    static constexpr int kTileH = 128;                         /* rows per tile */
    static constexpr int kBlocksX = kTileW / 8 + 1;            /* 13 / 9 offset block columns */
    static constexpr int kBlocksY = kTileH / 8 + 1;            /* 17 offset block rows */
    static constexpr int kLanes = kBlocksX * kBlocksY;         /* 221 / 153 */
    static constexpr int kComp = kBlocksX * 8 * SB;            /* 104 / 144 bytes of one component in a tile row */
    static constexpr int kPitch = 2 * kComp;                   /* 208 / 288 */
    static constexpr int kLds = (kTileH + 8) * kPitch;         /* 28288 / 39168 bytes: four workgroups per CU */
    static constexpr int kUnitsX = kTileW / 32, kUnits = kUnitsX * (kTileH / 32); /* 32 x 32 regions of stage 2: 12 / 8 */
};

/* tile accesses: 8 and 16 bytes at their natural alignment (ds_write_b64 / ds_read_b128 ...) */
struct alignas(8) W2 {
    uint32_t x, y;
};
struct alignas(16) W4 {
    uint32_t x, y, z, w;
};
DBK_HD W2 ld2(const uint8_t *p)
{
#if DBK_DEV
    return *reinterpret_cast<const W2 *>(p);
#else
    W2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
#endif
}
DBK_HD W4 ld4(const uint8_t *p)
{
#if DBK_DEV
    return *reinterpret_cast<const W4 *>(p);
#else
    W4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
#endif
}
DBK_HD void st2(uint8_t *p, uint32_t x, uint32_t y)
{
    const W2 v = {x, y};
#if DBK_DEV
    *reinterpret_cast<W2 *>(p) = v;
#else
    __builtin_memcpy(p, &v, 8);
#endif
}
DBK_HD void st4(uint8_t *p, const uint32_t (&w)[4])
{
    const W4 v = {w[0], w[1], w[2], w[3]};
#if DBK_DEV
    *reinterpret_cast<W4 *>(p) = v;
#else
    __builtin_memcpy(p, &v, 16);
#endif
}

/* ---- stage 1 of one lane: the block's eight rows of pairs as they came from memory (zeros for a half or a row outside the picture)
 * -> deblocked -> the two component tiles; (lbx, lby) = the block inside the tile ---- */
DBK_HD void deblock_to_tile(uint32_t (&D)[8][4], const dbk::H265Seg &cb, const dbk::H265Seg &cr, int /* max_v */, uint8_t *tile, int lbx, int lby)
{
    typedef Geo<1> G;
    uint32_t Lb[8], Rb[8], Lr[8], Rr[8];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        dbk::sp_split8<0>(D[r], Lb[r], Rb[r]);
        dbk::sp_split8<1>(D[r], Lr[r], Rr[r]);
    }
    dbk::packed_filter_block_h265<true>(Lb, Rb, cb);
    dbk::packed_filter_block_h265<true>(Lr, Rr, cr);
    uint8_t *const p = tile + (lby * 8) * G::kPitch + lbx * 8;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        st2(p + r * G::kPitch, Lb[r], Rb[r]);
        st2(p + r * G::kPitch + G::kComp, Lr[r], Rr[r]);
    }
}
DBK_HD void deblock_to_tile(uint32_t (&D)[8][8], const dbk::H265Seg &cb, const dbk::H265Seg &cr, int max_v, uint8_t *tile, int lbx, int lby)
{
    typedef Geo<2> G;
    uint32_t Wb[8][4], Wr[8][4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        dbk::sp_split16<0>(D[r], Wb[r]);
        dbk::sp_split16<1>(D[r], Wr[r]);
    }
    dbk::packed_filter_block16_h265<true>(Wb, cb, max_v);
    dbk::packed_filter_block16_h265<true>(Wr, cr, max_v);
    uint8_t *const p = tile + (lby * 8) * G::kPitch + lbx * 16;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        st4(p + r * G::kPitch, Wb[r]);
        st4(p + r * G::kPitch + G::kComp, Wr[r]);
    }
}

/* ---- stage 2 of one lane: SAO of the block of 8 pairs x 2 rows at tile position (qx, qy) = image (x, ys), inside one CTB and one
 * unit of the keep map, out of the two component tiles.  m = saonox::block_mask<2> of the block (the picture border included), with
 * saonox::W4 when the block is 4 pairs wide; masked = some lane of the wave has a mask (the wave's ballot): the masked procedure for
 * all of them.  store(r, d) takes output row r as the dwords of its pairs (4 for 8-bit samples, 8 for 16-bit containers); of a block
 * of 4 pairs the first half counts ---- */
struct Pic {
    int w, h;            /* samples per component */
    int ctb_log2, max_v, band_shift;
};

template <typename Store>
DBK_HD void sao_from_tile8(const uint8_t *tile, int qx, int qy, int x, int ys, const Pic &s, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept,
                           uint32_t m, bool masked, const Store &store)
{
    typedef Geo<1> G;
    /* image (x - 4, ys - 1 + i) is tile (column qx, row qy + 3 + i): the tile's origin is image (X0 - 4, Y0 - 4) */
    const uint8_t *const q0 = tile + (qy + 3) * G::kPitch + qx;
    auto fetch = [&](const uint8_t *q, int i) {
        const W2 lo = ld2(q + i * G::kPitch), hi = ld2(q + i * G::kPitch + 8);
        sao8::SaoRaw v;
        v.lh = lo.x; v.cx = lo.y; v.cy = hi.x; v.rh = hi.y;
        return v;
    };
    auto f0 = [&](int i, auto /* halo: the tile holds it anyway */) { return fetch(q0, i); };
    auto f1 = [&](int i, auto) { return fetch(q0 + G::kComp, i); };
    uint32_t O[2][2]; /* the first component's rows */
    auto s0 = [&](int r, uint32_t lo, uint32_t hi) { O[r][0] = lo; O[r][1] = hi; };
    auto s1 = [&](int r, uint32_t lo, uint32_t hi) {
        uint32_t d[4];
        dbk::sp_merge8(O[r][0], O[r][1], lo, hi, d);
        store(r, d);
    };
    if (!masked) {
        sao8::block<0, 2>(f0, s0, x, ys, s.w, s.h, c0, kept);
        sao8::block<0, 2>(f1, s1, x, ys, s.w, s.h, c1, kept);
    } else {
        sao8::block<2, 2, true>(f0, s0, x, ys, s.w, s.h, c0, kept, m);
        sao8::block<2, 2, true>(f1, s1, x, ys, s.w, s.h, c1, kept, m);
    }
}

template <typename Store>
DBK_HD void sao_from_tile16(const uint8_t *tile, int qx, int qy, int x, int ys, const Pic &s, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept,
                            uint32_t m, bool masked, const Store &store)
{
    typedef Geo<2> G;
    const uint8_t *const q0 = tile + (qy + 3) * G::kPitch + qx * 2;
    auto fetch = [&](const uint8_t *q, int i) {
        const W4 lo = ld4(q + i * G::kPitch), hi = ld4(q + i * G::kPitch + 16);
        sao16::Raw v;
        v.d[0] = lo.x; v.d[1] = lo.y; v.d[2] = lo.z; v.d[3] = lo.w; v.d[4] = hi.x; v.d[5] = hi.y; v.d[6] = hi.z; v.d[7] = hi.w;
        return v;
    };
    auto f0 = [&](int i, auto) { return fetch(q0, i); };
    auto f1 = [&](int i, auto) { return fetch(q0 + G::kComp, i); };
    uint32_t O[2][4];
    auto s0 = [&](int r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { O[r][0] = a; O[r][1] = b; O[r][2] = c; O[r][3] = d; };
    auto s1 = [&](int r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        const uint32_t w1[4] = {a, b, c, d};
        uint32_t o[8];
        dbk::sp_merge16(O[r], w1, o);
        store(r, o);
    };
    if (!masked) {
        sao16::block<0, 2>(f0, s0, x, ys, s.w, s.h, c0, kept, s.max_v, s.band_shift);
        sao16::block<0, 2>(f1, s1, x, ys, s.w, s.h, c1, kept, s.max_v, s.band_shift);
    } else {
        sao16::block<2, 2, true>(f0, s0, x, ys, s.w, s.h, c0, kept, s.max_v, s.band_shift, m);
        sao16::block<2, 2, true>(f1, s1, x, ys, s.w, s.h, c1, kept, s.max_v, s.band_shift, m);
    }
}

/* the block of lane l of the wave that works on unit u of the tile: its position inside the tile */
template <int SB>
DBK_HD void unit_block(int u, int l, int &qx, int &qy)
{
    const int uy = u / Geo<SB>::kUnitsX, ux = u - uy * Geo<SB>::kUnitsX;
    qx = ux * 32 + (l & 3) * 8;
    qy = uy * 32 + (l >> 2) * 2;
}

/* waves of a workgroup of `threads` lanes that share the tile's units evenly: 4 of 4 (256 lanes), 6 of 7 (448: 8-bit), 4 of 5 (320: 16-bit) */
template <int SB>
constexpr int sao_waves(int threads)
{
    int n = threads / 64;
    while (Geo<SB>::kUnits % n != 0) n--;
    return n;
}

} /* namespace spf */

#if defined(__HIPCC__)
#include "deblock_kernels.h"
#include "deblock_sp_dev.h"

namespace spf {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kOob = 0xfffffff0u; /* voffset >= num_records: load returns 0, store is dropped */

/* a 16-byte store with a scalar row offset is followed by two wait states before anything may write its data registers
 * (profiles/r04/store_hazard.md; deblock_sp.hip and sao_sp.hip do the same) */
__device__ __forceinline__ void store128(const u32x4 w, __amdgpu_buffer_rsrc_t rd, uint32_t voff, int soff)
{
    __builtin_amdgcn_raw_buffer_store_b128(w, rd, voff, soff, 0);
    asm volatile("s_nop 1" : : "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w) : "memory");
}

/* h.base.src -> s.dst; plane_w x plane_h, nbx / nby, the bS layouts, the CTB grid, the keep map and the boundary bytes are one
 * component's.  THREADS = the workgroup's size, at least Geo<SB>::kLanes; id = the workgroup's number inside this plane's part of the
 * grid, a multiple of 8 workgroups (fused_body) */
template <int SB, int THREADS>
__device__ __forceinline__ void body(const DbkH265Args &h, const DbkSaoArgs &s, const DbkFusedGrid &g, const DbkSaoCtb *params_cr, int cr_qp_offset,
                                     const DbkSaoNox &nx, const DbkSlOffs &sl, uint8_t *tile, uint32_t id)
{
    typedef Geo<SB> G;
    static_assert(THREADS >= G::kLanes && THREADS % 64 == 0, "one lane per offset block of the tile");
    const DbkArgs &a = h.base;
    /* each XCD works through a contiguous range of tiles (fused_body) */
    const uint32_t logical = (id & 7u) * g.per_xcd + (id >> 3);
    if (logical >= g.total) return; /* padding workgroup: the whole workgroup leaves before the barrier */
    const uint32_t fr = g.tiles_per_frame == 1u ? logical : __umulhi(logical, g.magic_tpf);
    const uint32_t in_frame = logical - fr * g.tiles_per_frame;
    const uint32_t trow = g.tiles_x == 1u ? in_frame : __umulhi(in_frame, g.magic_tx);
    const int t = (int)threadIdx.x, f = (int)fr;
    const int X0 = (int)(in_frame - trow * g.tiles_x) * G::kTileW, Y0 = (int)trow * G::kTileH;
    const int lby = t / G::kBlocksX; /* a constant divisor: multiply and shift */
    const int lbx = t - G::kBlocksX * lby;
    const bool in_tile = t < G::kLanes;
    const int bx = (X0 >> 3) + lbx, by = (Y0 >> 3) + lby;
    const bool active = in_tile && bx < a.nbx && by < a.nby;
    const bool lv = active && bx > 0, rv = active && dbk::g4_right_in(bx, a.plane_w);
    const bool full = lv && rv && by > 0 && dbk::g4_below_in(by, a.plane_h); /* all 8 rows and both halves inside the picture */
    const int y0 = by * 8 - 4;
    const uint32_t xoff = (uint32_t)(bx * 16 * SB - 8 * SB);
    const uint32_t plane_bytes = (uint32_t)a.pitch * (uint32_t)a.plane_h;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(a.src) + (long long)f * a.frame_stride, 0, plane_bytes, 0x00020000);

    /* ---- stage 1: this lane's offset block of pairs, HBM -> registers -> deblocked -> the two component tiles ---- */
    uint32_t D[8][4 * SB];
    if (__builtin_amdgcn_ballot_w64(active && !full) == 0ull) {
        /* no lane of the wave touches the picture border: 16-byte accesses, the row in the scalar offset */
        const uint32_t voff = full ? (uint32_t)y0 * (uint32_t)a.pitch + xoff : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, r * (int)a.pitch, 0);
            D[r][0] = w.x; D[r][1] = w.y; D[r][2] = w.z; D[r][3] = w.w;
            if constexpr (SB == 2) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, full ? voff + 16u : kOob, r * (int)a.pitch, 0);
                D[r][4] = v.x; D[r][5] = v.y; D[r][6] = v.z; D[r][7] = v.w;
            }
        }
    } else {
        /* the two halves of a row addressed separately; a half or a row outside the picture pushed out of the buffer's range */
        const uint32_t base = (uint32_t)(y0 * (int)a.pitch) + xoff;
        const uint32_t lbits = lv ? 0u : kOob, rbits = rv ? 0u : kOob;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const uint32_t ob = (unsigned)(y0 + r) < (unsigned)a.plane_h ? 0u : kOob;
            const uint32_t off = base + (uint32_t)r * (uint32_t)a.pitch;
            if constexpr (SB == 1) {
                const u32x2 l = __builtin_amdgcn_raw_buffer_load_b64(rs, off | lbits | ob, 0, 0);
                const u32x2 rr = __builtin_amdgcn_raw_buffer_load_b64(rs, (off + 8u) | rbits | ob, 0, 0);
                D[r][0] = l.x; D[r][1] = l.y; D[r][2] = rr.x; D[r][3] = rr.y;
            } else {
                const u32x4 l = __builtin_amdgcn_raw_buffer_load_b128(rs, off | lbits | ob, 0, 0);
                const u32x4 rr = __builtin_amdgcn_raw_buffer_load_b128(rs, (off + 16u) | rbits | ob, 0, 0);
                D[r][0] = l.x; D[r][1] = l.y; D[r][2] = l.z; D[r][3] = l.w;
                D[r][4] = rr.x; D[r][5] = rr.y; D[r][6] = rr.z; D[r][7] = rr.w;
            }
        }
    }
    /* the operands of an idle lane's block are those of block (0, 0): its rows are zeros, which every filter leaves alone */
    dbk::H265Seg cb, cr;
    dbk::sp_seg_params(h, sl, cr_qp_offset, f, active ? bx : 0, active ? by : 0, SB == 1 ? 0 : a.shift, SB == 1 ? 255 : a.max_v, cb, cr);
    if (in_tile) deblock_to_tile(D, cb, cr, a.max_v, tile, lbx, lby);
    __syncthreads();

    /* ---- stage 2: SAO of the tile out of LDS, one 32 x 32 region per wave at a time ---- */
    constexpr int NW = sao_waves<SB>(THREADS);
    const int wv = t >> 6, l = t & 63;
    if (wv >= NW) return;
    const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(s.dst + (long long)f * s.frame_stride, 0,
                                                                        (uint32_t)s.pitch * (uint32_t)s.plane_h, 0x00020000);
    const Pic pic = {s.plane_w, s.plane_h, s.ctb_log2, s.max_v, s.band_shift};
#pragma unroll 1
    for (int u = wv; u < G::kUnits; u += NW) {
        int qx, qy;
        unit_block<SB>(u, l, qx, qy);
        const int x = X0 + qx, ys = Y0 + qy;
        if (x >= s.plane_w || ys >= s.plane_h) continue;
        const uint32_t nox_byte = nx.nox ? saonox::ctb_byte(nx, f, x, ys, s.ctb_log2) : 0u; /* no bytes: nothing forbidden */
        const long long at = (long long)f * s.params_frame_stride + (long long)(ys >> s.ctb_log2) * s.params_stride + (x >> s.ctb_log2);
        const DbkSaoCtb c0 = s.params[at], c1 = params_cr[at];
        const bool kept = s.keep && s.keep[(long long)f * s.keep_frame_stride + (long long)(ys >> 3) * s.keep_stride + (x >> 3)];
        /* the last block of a row may be 4 pairs wide: on the picture border, so its wave takes the masked procedure anyway; the
         * picture's edge is behind its pair 3 (saonox::W4) and the first half of its rows alone is stored */
        const bool w4 = x + 8 > s.plane_w;
        const bool any_w4 = __builtin_amdgcn_ballot_w64(w4) != 0ull;
        const uint32_t m = saonox::block_mask<2>(nox_byte, x, ys, s.plane_w, s.plane_h, s.ctb_log2) | (w4 ? saonox::W4 : 0u);
        const bool masked = __builtin_amdgcn_ballot_w64(m != 0u) != 0ull;
        const uint32_t vout = (uint32_t)ys * (uint32_t)s.pitch + (uint32_t)x * (2u * SB);
        if constexpr (SB == 1) {
            auto store = [&](int r, const uint32_t (&d)[4]) {
                u32x4 w;
                w.x = d[0]; w.y = d[1]; w.z = d[2]; w.w = d[3];
                store128(w, rd, w4 ? kOob : vout, r * (int)s.pitch);
                if (any_w4) {
                    u32x2 hlf;
                    hlf.x = d[0]; hlf.y = d[1];
                    __builtin_amdgcn_raw_buffer_store_b64(hlf, rd, w4 ? vout : kOob, r * (int)s.pitch, 0);
                }
            };
            sao_from_tile8(tile, qx, qy, x, ys, pic, c0, c1, kept, m, masked, store);
        } else {
            auto store = [&](int r, const uint32_t (&d)[8]) {
                u32x4 w, v;
                w.x = d[0]; w.y = d[1]; w.z = d[2]; w.w = d[3];
                v.x = d[4]; v.y = d[5]; v.z = d[6]; v.w = d[7];
                store128(w, rd, vout, r * (int)s.pitch);
                store128(v, rd, w4 ? kOob : vout + 16u, r * (int)s.pitch);
            };
            sao_from_tile16(tile, qx, qy, x, ys, pic, c0, c1, kept, m, masked, store);
        }
    }
}

} /* namespace spf */
#endif /* __HIPCC__ */
