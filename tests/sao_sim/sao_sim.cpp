/*
 * sao_sim.cpp -- csrc/sao_packed.h compiled for the CPU (its device primitives emulated in the header's host branch), so that the
 * packed SAO arithmetic and the boundary-mask rule shared by the SAO pass and every fused deblocking + SAO kernel are checked
 * without a GPU.  tests/test_sao_sim_cpu.py builds this file with g++ (-I gpu_video_codec_amd/csrc) and drives it through ctypes.
 *
 *  - sao_sim_<primitive>: one primitive over its whole operand range, looped here, against a plain integer restatement of H.265
 *    8.7.3 written next to the loop.  The two 16-bit halves of every packed word carry DIFFERENT operands (one half walks the
 *    range, the other a pseudo-random sequence; then the halves swap), so that a carry or borrow from one half into the other
 *    shows.  out[0] = operand tuples visited, out[1] = mismatches, out[2..7] = the first mismatching operands.
 *  - sao_sim_plane: a whole plane in blocks of 8 x NROWS through sao8::block / sao16::block, the mask of each block from
 *    saonox::block_mask exactly as the fused kernel computes it; the plane is surrounded by poison, so that a result that depends
 *    on a sample outside the picture differs between two runs with different poison.
 */
#include <stdint.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "sao_packed.h"

namespace {

static_assert(sao8::kSel == 0x0c000c00u, "a selector half = the index in its low byte, 0x0c (constant zero) in its high byte");

/* ---- H.265 8.7.3.2 in plain integers ---- */
inline int sign(int v) { return (v > 0) - (v < 0); }
inline int clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
/* edgeIdx: 2 + Sign(rec - a) + Sign(rec - b), then (0, 1, 2) -> (1, 2, 0); 0 = no offset, k = SaoOffsetVal[k] */
inline int ref_edge_idx(int rec, int a, int b)
{
    int e = 2 + sign(rec - a) + sign(rec - b);
    if (e == 0 || e == 1 || e == 2) e = (e == 2) ? 0 : e + 1;
    return e;
}
/* bandTable[(k + sao_band_position) & 31] = k + 1, k = 0..3; bandIdx = bandTable[rec >> bandShift] */
inline int ref_band_idx(int rec, int shift, int pos)
{
    int table[32] = {0};
    for (int k = 0; k < 4; k++) table[(k + pos) & 31] = k + 1;
    return table[rec >> shift];
}
/* where the packed form keeps SaoOffsetVal[k] in its five-entry table.  Edge offset: 0 -> [1], 1 -> [2], 2 -> none, 3 -> [3],
 * 4 -> [4]; band offset: k - 1 -> [k], 4 -> none */
inline uint32_t edge_slot(int edge_idx) { return edge_idx == 0 ? 2u : (edge_idx <= 2 ? (uint32_t)edge_idx - 1u : (uint32_t)edge_idx); }
inline uint32_t band_slot(int band_idx) { return band_idx == 0 ? 4u : (uint32_t)band_idx - 1u; }
inline uint32_t sel_half(uint32_t slot) { return slot | 0x0c00u; }

inline uint32_t pack(uint32_t lo, uint32_t hi) { return (lo & 0xffffu) | (hi << 16); }
inline uint32_t next(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

struct Tally {
    uint64_t *out;
    explicit Tally(uint64_t *o) : out(o) { memset(o, 0, 8 * sizeof(uint64_t)); }
    void check(bool ok, uint64_t a, uint64_t b, uint64_t c, uint64_t d, uint64_t e, uint64_t f)
    {
        out[0]++;
        if (ok) return;
        if (out[1]++ == 0) { out[2] = a; out[3] = b; out[4] = c; out[5] = d; out[6] = e; out[7] = f; }
    }
};

/* edge_idx of operand triples p (one half) and q (the other half), both orders */
inline void edge_idx_both(Tally &t, const int (&p)[3], const int (&q)[3])
{
    for (int swap = 0; swap < 2; swap++) {
        const int(&lo)[3] = swap ? q : p;
        const int(&hi)[3] = swap ? p : q;
        const uint32_t got = sao8::edge_idx(pack(lo[0], hi[0]), pack(lo[1], hi[1]), pack(lo[2], hi[2]));
        const uint32_t want = pack(sel_half(edge_slot(ref_edge_idx(lo[0], lo[1], lo[2]))), sel_half(edge_slot(ref_edge_idx(hi[0], hi[1], hi[2]))));
        t.check(got == want, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]);
    }
}

/* a table of five offsets with `off` in slot idx and four other values around it; returns its biased bytes */
struct Table {
    int v[5];
    uint32_t lo, hi;
    Table(int idx, int off)
    {
        for (int k = 0; k < 5; k++) v[k] = (int)(int8_t)(off + 37 * (k - idx));
        auto b = [](int x) { return (uint32_t)(x + 128) & 0xffu; };
        lo = b(v[0]) | (b(v[1]) << 8) | (b(v[2]) << 16) | (b(v[3]) << 24);
        hi = b(v[4]);
    }
};

} /* namespace */

extern "C" {

/* sao8::edge_idx on 8-bit operands: all 2^24 (rec, a, b) x both orders */
void sao_sim_edge_idx8(uint64_t *out)
{
    Tally t(out);
    uint32_t s = 1u;
    for (int rec = 0; rec < 256; rec++)
        for (int a = 0; a < 256; a++)
            for (int b = 0; b < 256; b++) {
                const uint32_t r = next(s);
                const int p[3] = {rec, a, b}, q[3] = {(int)((r >> 8) & 255u), (int)((r >> 16) & 255u), (int)(r >> 24)};
                edge_idx_both(t, p, q);
            }
}

/* edge_idx on 16-bit operands (sao16 uses sao8's): all (rec, a) of 0..4095 x 0..4095, b of {0, rec - 1, rec, rec + 1, 4095} clipped, x both orders */
void sao_sim_edge_idx16(uint64_t *out)
{
    Tally t(out);
    uint32_t s = 2u;
    for (int rec = 0; rec < 4096; rec++)
        for (int a = 0; a < 4096; a++) {
            const int bs[5] = {0, clip3(0, 4095, rec - 1), rec, clip3(0, 4095, rec + 1), 4095};
            for (int i = 0; i < 5; i++) {
                const uint32_t r = next(s);
                const int p[3] = {rec, a, bs[i]}, q[3] = {(int)((r >> 8) & 4095u), (int)((r >> 20) & 4095u), (int)(((r >> 4) ^ (r >> 17)) & 4095u)};
                edge_idx_both(t, p, q);
            }
        }
}

/* sao8::apply: rec 0..255 x every int8 offset x index 0..4, x both orders */
void sao_sim_apply8(uint64_t *out)
{
    Tally t(out);
    uint32_t s = 3u;
    for (int rec = 0; rec < 256; rec++)
        for (int off = -128; off < 128; off++)
            for (int idx = 0; idx < 5; idx++) {
                const Table tab(idx, off);
                const uint32_t r = next(s);
                const int rec2 = (int)((r >> 8) & 255u), idx2 = (idx + 1 + (int)((r >> 20) & 3u)) % 5;
                for (int swap = 0; swap < 2; swap++) {
                    const int rl = swap ? rec2 : rec, il = swap ? idx2 : idx, rh = swap ? rec : rec2, ih = swap ? idx : idx2;
                    const uint32_t got = sao8::apply(pack(rl, rh), pack(sel_half(il), sel_half(ih)), tab.lo, tab.hi);
                    const uint32_t want = pack(clip3(0, 255, rl + tab.v[il]), clip3(0, 255, rh + tab.v[ih]));
                    t.check(got == want, rl, il, tab.v[il], rh, ih, tab.v[ih]);
                }
            }
}

/* sao16::apply: bit depth 8..12, rec 0..max_v x every int8 offset x index 0..4 with maxv of that depth, x both orders */
void sao_sim_apply16(uint64_t *out)
{
    Tally t(out);
    uint32_t s = 4u;
    for (int depth = 8; depth <= 12; depth++) {
        const int max_v = (1 << depth) - 1;
        for (int rec = 0; rec <= max_v; rec++)
            for (int off = -128; off < 128; off++)
                for (int idx = 0; idx < 5; idx++) {
                    const Table tab(idx, off);
                    const sao16::Tab tb = {tab.lo, tab.hi, (uint32_t)max_v * 0x00010001u};
                    const uint32_t r = next(s);
                    const int rec2 = (int)((r >> 8) & (uint32_t)max_v), idx2 = (idx + 1 + (int)((r >> 22) & 3u)) % 5;
                    for (int swap = 0; swap < 2; swap++) {
                        const int rl = swap ? rec2 : rec, il = swap ? idx2 : idx, rh = swap ? rec : rec2, ih = swap ? idx : idx2;
                        const uint32_t got = sao16::apply(pack(rl, rh), pack(sel_half(il), sel_half(ih)), tb);
                        const uint32_t want = pack(clip3(0, max_v, rl + tab.v[il]), clip3(0, max_v, rh + tab.v[ih]));
                        t.check(got == want, rl, il, tab.v[il], rh, ih, (uint64_t)depth << 32 | (uint32_t)tab.v[ih]);
                    }
                }
    }
}

/* sao8::band_sel: shift 3..7 (bit depth shift + 5), every rec of that depth x position 0..31, x both orders */
void sao_sim_band_sel(uint64_t *out)
{
    Tally t(out);
    uint32_t s = 5u;
    for (int shift = 3; shift <= 7; shift++) {
        const int max_v = (1 << (shift + 5)) - 1;
        for (int rec = 0; rec <= max_v; rec++)
            for (int pos = 0; pos < 32; pos++) {
                const int rec2 = (int)((next(s) >> 8) & (uint32_t)max_v);
                for (int swap = 0; swap < 2; swap++) {
                    const int rl = swap ? rec2 : rec, rh = swap ? rec : rec2;
                    const uint32_t got = sao8::band_sel(pack(rl, rh), shift, sao8::s_splat(pos));
                    const uint32_t want = pack(sel_half(band_slot(ref_band_idx(rl, shift, pos))), sel_half(band_slot(ref_band_idx(rh, shift, pos))));
                    t.check(got == want, rl, rh, shift, pos, got, want);
                }
            }
    }
}

/* saonox::block_mask<NROWS> itself, for a look at single blocks */
uint32_t sao_sim_block_mask(int nrows, uint32_t byte, int x, int y0, int w, int h, int ctb_log2)
{
    if (nrows == 2) return saonox::block_mask<2>(byte, x, y0, w, h, ctb_log2);
    if (nrows == 4) return saonox::block_mask<4>(byte, x, y0, w, h, ctb_log2);
    return saonox::block_mask<8>(byte, x, y0, w, h, ctb_log2);
}

} /* extern "C" */

/* ---- whole planes ------------------------------------------------------------------------------------------------------------ */
namespace {

struct PlaneArgs {
    const void *src;
    void *dst; /* h rows of w samples each, no padding */
    int w, h, bit_depth;
    const DbkSaoCtb *params;
    int params_stride, ctb_log2;
    const uint8_t *keep;
    int keep_stride;
    DbkSaoNox nx; /* nx.nox == NULL: no bytes */
    int border;   /* 1: the picture border alone (block<1>); 2: the block's mask (block<2>) */
    int force;    /* 0: a block whose own mask / border flag is zero takes block<0>, as in a wave none of whose lanes is on a border;
                     1: it takes the bordered form, as in a wave with such a lane */
    int poison;
};

constexpr int kMarginX = 8, kMarginTop = 2, kMarginRight = 16, kMarginBottom = 12;

template <typename T, int NROWS, bool G4>
int run_plane(const PlaneArgs &a)
{
    const int w = a.w, h = a.h, pw = w + kMarginX + kMarginRight, ph = h + kMarginTop + kMarginBottom;
    std::vector<T> pad((size_t)pw * ph, (T)a.poison);
    for (int y = 0; y < h; y++) memcpy(&pad[(size_t)(y + kMarginTop) * pw + kMarginX], (const T *)a.src + (size_t)y * w, (size_t)w * sizeof(T));
    T *const dst = (T *)a.dst;
    const int max_v = (1 << a.bit_depth) - 1, band_shift = a.bit_depth - 5;
    int bad_store = 0;
    for (int y0 = 0; y0 < h; y0 += NROWS)
        for (int x = 0; x < w; x += 8) {
            const DbkSaoCtb c = a.params[(long long)(y0 >> a.ctb_log2) * a.params_stride + (x >> a.ctb_log2)];
            const bool kept = a.keep && a.keep[(long long)(y0 >> 3) * a.keep_stride + (x >> 3)];
            const uint32_t nox_byte = a.nx.nox ? saonox::ctb_byte(a.nx, 0, x, y0, a.ctb_log2) : 0u;
            const bool w4 = G4 && x + 8 > w, h4 = G4 && NROWS == 8 && y0 + 8 > h;
            /* raw row i = image row y0 - 1 + i, samples x - 4 .. x + 11 */
            const T *const q0 = &pad[(size_t)(y0 - 1 + kMarginTop) * pw + (x - 4 + kMarginX)];
            auto put = [&](int r, const uint32_t *d, int n_dwords) {
                const int n = w4 ? n_dwords / 2 : n_dwords; /* a block of 4 samples stores its low half alone */
                if (y0 + r >= h || x + n * (int)(4 / sizeof(T)) > w) { bad_store++; return; }
                memcpy(dst + (size_t)(y0 + r) * w + x, d, (size_t)n * 4);
            };
            uint32_t m = 0u;
            bool own;
            if (a.border == 2) {
                m = (h4 ? saonox::block_mask<4>(nox_byte, x, y0, w, h, a.ctb_log2) : saonox::block_mask<NROWS>(nox_byte, x, y0, w, h, a.ctb_log2)) |
                    (w4 ? saonox::W4 : 0u);
                own = m != 0u;
            } else {
                own = x == 0 || x + 8 == w || y0 == 0 || y0 + NROWS >= h;
            }
            const bool bordered = own || a.force;
            if constexpr (sizeof(T) == 1) {
                auto fetch = [&](int i, auto) {
                    sao8::SaoRaw q;
                    uint32_t d[4];
                    memcpy(d, q0 + (size_t)i * pw, 16);
                    q.lh = d[0]; q.cx = d[1]; q.cy = d[2]; q.rh = d[3];
                    return q;
                };
                auto store = [&](int r, uint32_t lo, uint32_t hi) {
                    const uint32_t d[2] = {lo, hi};
                    put(r, d, 2);
                };
                if (!bordered) sao8::block<0, NROWS, false>(fetch, store, x, y0, w, h, c, kept);
                else if (a.border == 1) sao8::block<1, NROWS, false>(fetch, store, x, y0, w, h, c, kept);
                else if (h4) sao8::block<2, 4, G4>(fetch, store, x, y0, w, h, c, kept, m);
                else sao8::block<2, NROWS, G4>(fetch, store, x, y0, w, h, c, kept, m);
            } else {
                auto fetch = [&](int i, auto) {
                    sao16::Raw q;
                    memcpy(q.d, q0 + (size_t)i * pw, 32);
                    return q;
                };
                auto store = [&](int r, uint32_t d0, uint32_t d1, uint32_t d2, uint32_t d3) {
                    const uint32_t d[4] = {d0, d1, d2, d3};
                    put(r, d, 4);
                };
                if (!bordered) sao16::block<0, NROWS, false>(fetch, store, x, y0, w, h, c, kept, max_v, band_shift);
                else if (a.border == 1) sao16::block<1, NROWS, false>(fetch, store, x, y0, w, h, c, kept, max_v, band_shift);
                else if (h4) sao16::block<2, 4, G4>(fetch, store, x, y0, w, h, c, kept, max_v, band_shift, m);
                else sao16::block<2, NROWS, G4>(fetch, store, x, y0, w, h, c, kept, max_v, band_shift, m);
            }
        }
    return bad_store ? -2 : 0;
}

} /* namespace */

extern "C" int sao_sim_plane(const void *src, void *dst, int w, int h, int sample_bytes, int bit_depth, const DbkSaoCtb *params, int params_stride,
                             int ctb_log2, const uint8_t *keep, int keep_stride, const uint8_t *nox, int nox_stride, int border, int force,
                             int nrows, int g4, int poison)
{
    const int unit = g4 ? 4 : 8;
    if (w <= 0 || h <= 0 || w % unit || h % unit || (sample_bytes != 1 && sample_bytes != 2) || (border != 1 && border != 2) ||
        (nrows != 8 && nrows != 2) || (g4 && border != 2) || ctb_log2 < 3)
        return -1;
    PlaneArgs a = {src, dst, w, h, bit_depth, params, params_stride, ctb_log2, keep, keep_stride, {nox, nox_stride, 0}, border, force, poison};
    if (sample_bytes == 1) {
        if (g4) return nrows == 8 ? run_plane<uint8_t, 8, true>(a) : run_plane<uint8_t, 2, true>(a);
        return nrows == 8 ? run_plane<uint8_t, 8, false>(a) : run_plane<uint8_t, 2, false>(a);
    }
    if (g4) return nrows == 8 ? run_plane<uint16_t, 8, true>(a) : run_plane<uint16_t, 2, true>(a);
    return nrows == 8 ? run_plane<uint16_t, 8, false>(a) : run_plane<uint16_t, 2, false>(a);
}
