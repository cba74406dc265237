/*
 * sao_sp_sim.cpp -- runs the semi-planar SAO KERNELS' per-block procedures (gpu_video_codec_amd/csrc/sao_sp.h: deblock_sp.h's split
 * and merge around the packed block procedures of sao_packed.h, and the per-sample procedure with a component stride of 2) on the CPU
 * over a whole plane of interleaved Cb / Cr pairs, wave by wave as sao_sp.hip does: a 64 x 64 region whose blocks' masks
 * (saonox::block_mask) are all zero runs BORDER = 0, a region holding a block of 4 columns or 4 rows the per-sample procedure, every
 * other region BORDER = 2.  The loads are the kernels': raw row j at the clamped row, halo dwords outside a row moved inside it, and
 * -- like a buffer resource -- zero for anything outside pitch * plane_h.  TEST-ONLY: built by tests/test_sao_sp_cpu.py, never part of
 * the product library.
 */
#include <cstdint>
#include <cstring>

#include "../../gpu_video_codec_amd/csrc/sao_sp.h"

namespace {

struct Job {
    const uint8_t *src;
    uint8_t *dst;
    long pitch;
    int w, h, ctb_log2, max_v, band_shift;
    const DbkSaoCtb *pcb, *pcr;
    int pstride;
    const uint8_t *keep;
    int keep_stride;
    const uint8_t *nox;
    int nox_stride;
};

/* SB = bytes per sample */
template <int SB, int BORDER>
void packed_block(const Job &j, int x, int y0, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept, uint32_t m)
{
    const long bytes = j.pitch * j.h, bx = (long)x * 2 * SB;
    auto rd32 = [&](long off) {
        uint32_t v = 0u;
        if (off >= 0 && off + 4 <= bytes) std::memcpy(&v, j.src + off, 4);
        return v;
    };
    auto at = [&](int r) {
        int y = y0 - 1 + r;
        if (BORDER != 0) y = y < 0 ? 0 : (y >= j.h ? j.h - 1 : y);
        return (long)y * j.pitch + bx;
    };
    auto load = [&](int r, uint32_t (&d)[4 * SB], uint32_t &hl, uint32_t &hr, bool halo) {
        const long o = at(r);
        for (int i = 0; i < 4 * SB; i++) d[i] = rd32(o + 4 * i);
        if (halo) {
            long lo = o - 4, ro = o + 16 * SB;
            if (BORDER != 0) {
                if (x == 0) lo = o;
                if (x + 8 >= j.w) ro = o + 16 * SB - 4;
            }
            hl = rd32(lo);
            hr = rd32(ro);
        }
    };
    auto store = [&](int r, const uint32_t (&d)[4 * SB]) { std::memcpy(j.dst + (long)(y0 + r) * j.pitch + bx, d, 16 * SB); };
    if constexpr (SB == 1) saosp::block8<BORDER>(load, store, x, y0, j.w, j.h, c0, c1, kept, m);
    else saosp::block16<BORDER>(load, store, x, y0, j.w, j.h, c0, c1, kept, j.max_v, j.band_shift, m);
}

template <typename T>
void run(const Job &j, int form)
{
    constexpr int SB = (int)sizeof(T);
    const saosp::Plane pl = {j.src, j.dst, j.pitch, j.w, j.h, j.ctb_log2, j.max_v, j.band_shift};
    for (int wy = 0; wy < j.h; wy += 64)
        for (int wx = 0; wx < j.w; wx += 64) {
            /* the wave's two ballots */
            bool any_mask = false, any_short = false;
            for (int y0 = wy; y0 < wy + 64 && y0 < j.h; y0 += 8)
                for (int x = wx; x < wx + 64 && x < j.w; x += 8) {
                    const uint32_t b = j.nox ? j.nox[(long)(y0 >> j.ctb_log2) * j.nox_stride + (x >> j.ctb_log2)] : 0u;
                    any_mask |= saonox::block_mask<8>(b, x, y0, j.w, j.h, j.ctb_log2) != 0u;
                    any_short |= x + 8 > j.w || y0 + 8 > j.h;
                }
            for (int y0 = wy; y0 < wy + 64 && y0 < j.h; y0 += 8)
                for (int x = wx; x < wx + 64 && x < j.w; x += 8) {
                    const long at = (long)(y0 >> j.ctb_log2) * j.pstride + (x >> j.ctb_log2);
                    const uint32_t b = j.nox ? j.nox[(long)(y0 >> j.ctb_log2) * j.nox_stride + (x >> j.ctb_log2)] : 0u;
                    const bool kept = j.keep && j.keep[(long)(y0 >> 3) * j.keep_stride + (x >> 3)];
                    const uint32_t m = saonox::block_mask<8>(b, x, y0, j.w, j.h, j.ctb_log2);
                    if (form == 0 || (any_mask && any_short)) saosp::block_px<T>(pl, b, x, y0, j.pcb[at], j.pcr[at], kept);
                    else if (!any_mask) packed_block<SB, 0>(j, x, y0, j.pcb[at], j.pcr[at], kept, m);
                    else packed_block<SB, 2>(j, x, y0, j.pcb[at], j.pcr[at], kept, m);
                }
        }
}

} /* namespace */

/* w x h = the samples per component; src / dst hold 2 * w samples per row at `pitch` bytes.  form 0 = the per-sample kernel, 1 = the
 * packed kernels (up to 12 bit) */
extern "C" int sao_sp_sim_plane(const void *src, void *dst, int w, int h, long pitch, int sample_bytes, int bit_depth, const void *pcb,
                                const void *pcr, int pstride, int ctb_log2, const uint8_t *keep, int keep_stride, const uint8_t *nox,
                                int nox_stride, int form)
{
    if (w < 8 || h < 8 || w % 4 || h % 4) return 2;
    if (form == 1 && bit_depth > 12) return 3;
    const Job j = {(const uint8_t *)src, (uint8_t *)dst, pitch, w, h, ctb_log2, (1 << bit_depth) - 1, bit_depth - 5,
                   (const DbkSaoCtb *)pcb, (const DbkSaoCtb *)pcr, pstride, keep, keep_stride, nox, nox_stride};
    if (sample_bytes == 1) run<uint8_t>(j, form);
    else run<uint16_t>(j, form);
    return 0;
}
