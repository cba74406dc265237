/*
 * sao_sp.h -- sample adaptive offset (H.265 8.7.3) of one 8x8 block of sample PAIRS of a semi-planar chroma plane (interleaved Cb / Cr:
 * the _sp SAO entries of the C ABI).  The block's rows are taken apart by deblock_sp.h's selectors into the raw rows the packed block
 * procedures of sao_packed.h work on, the procedures run once per component with that component's CTB entry, and the two results go
 * back through the merge into ONE row piece per row.
 *
 * A lane's row piece is 16 bytes (8-bit samples) or 32 bytes (16-bit containers); the halo of the classes with horizontal neighbours
 * is one PAIR to the left and one to the right, i.e. the dword in front of the piece and the dword behind it, of which each
 * component looks at one sample.  The ten rows y0 - 1 .. y0 + 8 are fetched ONCE, into registers, and serve both components: the
 * procedures are used as they are (their fetch functor then reads registers), so the first component's eight output rows wait in
 * registers (16 / 32 VGPRs) until the second component's row is there to be merged with -- running the two in lockstep would need a
 * block procedure of its own.
 *
 * Where the two components agree in type and, for edge offset, in class (what H.265 7.3.8.3 gives every CTB of a stream) the class
 * is resolved once and both run the same instantiation; any other two entries run the general procedure one after the other.
 *
 * block_px: the per-sample procedure with a component stride of 2 -- samples deeper than 12 bit, planes the packed kernels refuse,
 * and the blocks of 4 columns / 4 rows of a plane whose sizes are multiples of 4.
 *
 * DBK_HD like sao_packed.h: tests/sao_sp_sim runs all of this on the CPU against tests/sao_sp_ref.py.
 */
#pragma once
#include "sao_packed.h"
#include "deblock_sp.h"

namespace saosp {

/* ---- the packed forms ---- */

/* the four dwords of a row piece and its two halo dwords -> component C's raw row.  hl = the pairs x-2, x-1 (bytes Cb Cr Cb Cr), hr =
 * the pairs x+8, x+9: sao8 looks at byte 3 of lh (sample x-1) and byte 0 of rh (sample x+8) only */
template <int C>
DBK_HD sao8::SaoRaw raw8(const uint32_t (&d)[4], uint32_t hl, uint32_t hr)
{
    sao8::SaoRaw q;
    dbk::sp_split8<C>(d, q.cx, q.cy);
    q.lh = C == 0 ? hl << 8 : hl;
    q.rh = C == 0 ? hr : hr >> 8;
    return q;
}
/* 16-bit containers: hl = the pair x-1 (Cb in the low half), hr = the pair x+8; sao16 looks at the high half of d[1] and the low
 * half of d[6] */
template <int C>
DBK_HD sao16::Raw raw16(const uint32_t (&d)[8], uint32_t hl, uint32_t hr)
{
    sao16::Raw q;
    uint32_t w[4];
    dbk::sp_split16<C>(d, w);
    q.d[0] = q.d[7] = 0u;
    q.d[1] = C == 0 ? hl << 16 : hl;
    q.d[2] = w[0]; q.d[3] = w[1]; q.d[4] = w[2]; q.d[5] = w[3];
    q.d[6] = C == 0 ? hr : hr >> 16;
    return q;
}

DBK_HD bool is_edge(const DbkSaoCtb &c) { return c.type == 2; }
DBK_HD bool looks_sideways(const DbkSaoCtb &c) { return c.type == 2 && (c.cls & 3) != 1; }
DBK_HD uint32_t bias(int v) { return (uint32_t)(v + 128) & 0xffu; }

/* One block of 8 x 8 pairs of 8-bit samples at (x, y0), inside one CTB.  load(j, d, hl, hr, halo) fills raw row j = image row
 * y0 - 1 + j (j = 0 and 9 are asked for only when a component is edge offset, the halo dwords only when `halo`); store(r, d) takes
 * output row r as its four dwords.  BORDER 0: no lane of the wave has a direction it must not look in; 2: m = saonox::block_mask */
template <int BORDER, typename Load, typename Store>
DBK_HD void block8(const Load &load, const Store &store, int x, int y0, int w, int h, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept,
                   uint32_t m)
{
    const bool e0 = !kept && is_edge(c0), e1 = !kept && is_edge(c1);
    const bool edge = e0 || e1, halo = !kept && (looks_sideways(c0) || looks_sideways(c1));
    uint32_t D[10][4], HL[10], HR[10];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 10; j++) {
        D[j][0] = D[j][1] = D[j][2] = D[j][3] = HL[j] = HR[j] = 0u;
        if (edge || (j >= 1 && j <= 8)) load(j, D[j], HL[j], HR[j], halo);
    }
    uint32_t O[8][2]; /* the first component's rows */
    auto f0 = [&](int j, auto) { return raw8<0>(D[j], HL[j], HR[j]); };
    auto f1 = [&](int j, auto) { return raw8<1>(D[j], HL[j], HR[j]); };
    auto s0 = [&](int r, uint32_t lo, uint32_t hi) { O[r][0] = lo; O[r][1] = hi; };
    auto s1 = [&](int r, uint32_t lo, uint32_t hi) {
        uint32_t d[4];
        dbk::sp_merge8(O[r][0], O[r][1], lo, hi, d);
        store(r, d);
    };
    if (e0 && e1 && ((c0.cls ^ c1.cls) & 3) == 0) { /* the conformant edge-offset CTB: one class for both */
        const uint32_t a_lo = bias(c0.offset[0]) | (bias(c0.offset[1]) << 8) | (bias(0) << 16) | (bias(c0.offset[2]) << 24), a_hi = bias(c0.offset[3]);
        const uint32_t b_lo = bias(c1.offset[0]) | (bias(c1.offset[1]) << 8) | (bias(0) << 16) | (bias(c1.offset[2]) << 24), b_hi = bias(c1.offset[3]);
        const int cls = c0.cls & 3;
        if (cls == 0) {
            sao8::edge_rows<0, BORDER, 8>(f0, s0, x, y0, w, h, a_lo, a_hi, m);
            sao8::edge_rows<0, BORDER, 8>(f1, s1, x, y0, w, h, b_lo, b_hi, m);
        } else if (cls == 1) {
            sao8::edge_rows<1, BORDER, 8>(f0, s0, x, y0, w, h, a_lo, a_hi, m);
            sao8::edge_rows<1, BORDER, 8>(f1, s1, x, y0, w, h, b_lo, b_hi, m);
        } else if (cls == 2) {
            sao8::edge_rows<2, BORDER, 8>(f0, s0, x, y0, w, h, a_lo, a_hi, m);
            sao8::edge_rows<2, BORDER, 8>(f1, s1, x, y0, w, h, b_lo, b_hi, m);
        } else {
            sao8::edge_rows<3, BORDER, 8>(f0, s0, x, y0, w, h, a_lo, a_hi, m);
            sao8::edge_rows<3, BORDER, 8>(f1, s1, x, y0, w, h, b_lo, b_hi, m);
        }
        return;
    }
    sao8::block<BORDER, 8>(f0, s0, x, y0, w, h, c0, kept, m);
    sao8::block<BORDER, 8>(f1, s1, x, y0, w, h, c1, kept, m);
}

/* the same for 16-bit containers up to 12 bit: d = eight dwords, hl / hr = the dwords at -4 and +32 */
template <int BORDER, typename Load, typename Store>
DBK_HD void block16(const Load &load, const Store &store, int x, int y0, int w, int h, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept,
                    int max_v, int band_shift, uint32_t m)
{
    const bool e0 = !kept && is_edge(c0), e1 = !kept && is_edge(c1);
    const bool edge = e0 || e1, halo = !kept && (looks_sideways(c0) || looks_sideways(c1));
    uint32_t D[10][8], HL[10], HR[10];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 10; j++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int i = 0; i < 8; i++) D[j][i] = 0u;
        HL[j] = HR[j] = 0u;
        if (edge || (j >= 1 && j <= 8)) load(j, D[j], HL[j], HR[j], halo);
    }
    uint32_t O[8][4];
    auto f0 = [&](int j, auto) { return raw16<0>(D[j], HL[j], HR[j]); };
    auto f1 = [&](int j, auto) { return raw16<1>(D[j], HL[j], HR[j]); };
    auto s0 = [&](int r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { O[r][0] = a; O[r][1] = b; O[r][2] = c; O[r][3] = d; };
    auto s1 = [&](int r, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
        const uint32_t w1[4] = {a, b, c, d};
        uint32_t o[8];
        dbk::sp_merge16(O[r], w1, o);
        store(r, o);
    };
    if (e0 && e1 && ((c0.cls ^ c1.cls) & 3) == 0) {
        sao16::Tab ta, tb;
        ta.maxv = tb.maxv = (uint32_t)max_v * 0x00010001u;
        ta.lo = bias(c0.offset[0]) | (bias(c0.offset[1]) << 8) | (0x80u << 16) | (bias(c0.offset[2]) << 24); ta.hi = bias(c0.offset[3]);
        tb.lo = bias(c1.offset[0]) | (bias(c1.offset[1]) << 8) | (0x80u << 16) | (bias(c1.offset[2]) << 24); tb.hi = bias(c1.offset[3]);
        const int cls = c0.cls & 3;
        if (cls == 0) {
            sao16::edge_rows<0, BORDER, 8>(f0, s0, x, y0, w, h, ta, m);
            sao16::edge_rows<0, BORDER, 8>(f1, s1, x, y0, w, h, tb, m);
        } else if (cls == 1) {
            sao16::edge_rows<1, BORDER, 8>(f0, s0, x, y0, w, h, ta, m);
            sao16::edge_rows<1, BORDER, 8>(f1, s1, x, y0, w, h, tb, m);
        } else if (cls == 2) {
            sao16::edge_rows<2, BORDER, 8>(f0, s0, x, y0, w, h, ta, m);
            sao16::edge_rows<2, BORDER, 8>(f1, s1, x, y0, w, h, tb, m);
        } else {
            sao16::edge_rows<3, BORDER, 8>(f0, s0, x, y0, w, h, ta, m);
            sao16::edge_rows<3, BORDER, 8>(f1, s1, x, y0, w, h, tb, m);
        }
        return;
    }
    sao16::block<BORDER, 8>(f0, s0, x, y0, w, h, c0, kept, max_v, band_shift, m);
    sao16::block<BORDER, 8>(f1, s1, x, y0, w, h, c1, kept, max_v, band_shift, m);
}

/* ---- the per-sample form ---- */

/* one word of four samples = two pairs */
template <typename T>
struct Word;
template <>
struct Word<uint8_t> {
    typedef uint32_t W;
    static DBK_HD void unpack(W w, int (&o)[4]) { o[0] = w & 0xff; o[1] = (w >> 8) & 0xff; o[2] = (w >> 16) & 0xff; o[3] = w >> 24; }
    static DBK_HD W pack(const int (&o)[4]) { return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24); }
};
template <>
struct Word<uint16_t> {
    struct alignas(8) W { uint32_t x, y; };
    static DBK_HD void unpack(W w, int (&o)[4]) { o[0] = w.x & 0xffff; o[1] = w.x >> 16; o[2] = w.y & 0xffff; o[3] = w.y >> 16; }
    static DBK_HD W pack(const int (&o)[4]) { return W{(uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)}; }
};

DBK_HD int sgn(int v) { return (v > 0) - (v < 0); }

/* the bit of a CTB's boundary byte that speaks for the neighbouring CTB (dcx, dcy), each -1 / 0 / 1; (0, 0): none */
DBK_HD uint32_t nox_bit(int dcx, int dcy)
{
    using namespace saonox;
    return dcy < 0 ? (dcx < 0 ? UL : (dcx > 0 ? UR : U)) : (dcy > 0 ? (dcx < 0 ? DL : (dcx > 0 ? DR : D)) : (dcx < 0 ? L : (dcx > 0 ? R : 0u)));
}

struct Plane {
    const uint8_t *src; /* one frame */
    uint8_t *dst;
    long long pitch;  /* bytes */
    int w, h;         /* samples per component */
    int ctb_log2, max_v, band_shift;
};

/* One block of 8 or 4 pairs by 8 or 4 rows at (x, y0), the short ones being the last of their row / column of blocks: every sample
 * tested against the picture and against the CTB's boundary byte `nox`, as the planar _g4 kernels' per-sample procedure does it, on the
 * samples 2 (x + i) + k of a row for component k.  Both components of a row leave in the same words; nothing beyond 2 w samples of a
 * row is read or written */
template <typename T>
DBK_HD void block_px(const Plane &p, uint32_t nox, int x, int y0, const DbkSaoCtb &c0, const DbkSaoCtb &c1, bool kept)
{
    typedef typename Word<T>::W W;
    const bool w8 = x + 8 <= p.w;
    const int nr = y0 + 8 <= p.h ? 8 : 4;
    const long long bx = (long long)x * 2 * (int)sizeof(T); /* the block's byte offset in a row */
    auto row_at = [&](int y) { return p.src + (long long)(y < 0 ? 0 : (y >= p.h ? p.h - 1 : y)) * p.pitch; };
    /* v[k][0..9] = samples x-1 .. x+8 of component k; positions outside the row hold junk that no sample inside the picture uses */
    auto ld = [&](const uint8_t *row, int (&v)[2][10]) {
        int q[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++) {
            if (j < 2 || w8) Word<T>::unpack(*reinterpret_cast<const W *>(row + bx + 4 * j * (int)sizeof(T)), q);
            else q[0] = q[1] = q[2] = q[3] = 0;
            v[0][1 + 2 * j] = q[0]; v[1][1 + 2 * j] = q[1]; v[0][2 + 2 * j] = q[2]; v[1][2 + 2 * j] = q[3];
        }
        Word<T>::unpack(*reinterpret_cast<const W *>(row + (x >= 4 ? bx - 4 * (int)sizeof(T) : 0)), q);
        v[0][0] = q[2]; v[1][0] = q[3];
        Word<T>::unpack(*reinterpret_cast<const W *>(row + (x + 8 < p.w ? bx + 16 * (int)sizeof(T) : (long long)(2 * p.w - 4) * (int)sizeof(T))), q);
        v[0][9] = q[0]; v[1][9] = q[1];
    };
    auto st = [&](uint8_t *row, const int (&o)[2][8]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int j = 0; j < 4; j++)
            if (j < 2 || w8) {
                const int q[4] = {o[0][2 * j], o[1][2 * j], o[0][2 * j + 1], o[1][2 * j + 1]};
                *reinterpret_cast<W *>(row + bx + 4 * j * (int)sizeof(T)) = Word<T>::pack(q);
            }
    };
    if (kept || (c0.type != 2 && c1.type != 2)) {
        /* neither component looks at a neighbour: the block's own rows only, copied or band offset (what sao_block_g4 does for them) */
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int r = 0; r < 8; r++) {
            if (r < nr) {
                const uint8_t *row = p.src + (long long)(y0 + r) * p.pitch;
                int o[2][8];
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int j = 0; j < 4; j++) {
                    int q[4] = {0, 0, 0, 0};
                    if (j < 2 || w8) Word<T>::unpack(*reinterpret_cast<const W *>(row + bx + 4 * j * (int)sizeof(T)), q);
                    o[0][2 * j] = q[0]; o[1][2 * j] = q[1]; o[0][2 * j + 1] = q[2]; o[1][2 * j + 1] = q[3];
                }
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int k = 0; k < 2; k++) {
                    const DbkSaoCtb &c = k ? c1 : c0;
                    if (!kept && c.type == 1) { /* band offset: bandTable[(k + sao_band_position) & 31] = k + 1 */
#if defined(__HIPCC__)
#pragma unroll
#endif
                        for (int i = 0; i < 8; i++) {
                            const int b = ((o[k][i] >> p.band_shift) - (int)c.cls) & 31;
                            const int v = o[k][i] + (b == 0 ? c.offset[0] : (b == 1 ? c.offset[1] : (b == 2 ? c.offset[2] : (b == 3 ? c.offset[3] : 0))));
                            o[k][i] = v < 0 ? 0 : (v > p.max_v ? p.max_v : v);
                        }
                    }
                }
                st(p.dst + (long long)(y0 + r) * p.pitch, o);
            }
        }
        return;
    }
    int up[2][10], mid[2][10], dn[2][10];
    ld(row_at(y0 - 1), up);
    ld(row_at(y0), mid);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 8; r++) {
        if (r < nr) {
            const int y = y0 + r;
            ld(row_at(y + 1), dn);
            int o[2][8];
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 2; k++) {
                const DbkSaoCtb &c = k ? c1 : c0;
                const int cls = c.cls & 3;
                const int dxa = cls == 1 ? 0 : (cls == 3 ? 1 : -1);
                const bool vertical = cls != 0;
                const int dya = vertical ? -1 : 0;
                const bool rows_ok = !vertical || (y > 0 && y < p.h - 1);
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int i = 0; i < 8; i++) {
                    const int rec = mid[k][1 + i];
                    int off = 0;
                    const bool copy = kept || c.type == 0 || c.type > 2;
                    if (copy) {
                        off = 0;
                    } else if (c.type == 1) { /* band offset: bandTable[(k + sao_band_position) & 31] = k + 1 */
                        const int b = ((rec >> p.band_shift) - (int)c.cls) & 31;
                        off = b == 0 ? c.offset[0] : (b == 1 ? c.offset[1] : (b == 2 ? c.offset[2] : (b == 3 ? c.offset[3] : 0)));
                    } else { /* edge offset, Table 8-13 */
                        const int xa = x + i + dxa, xb = x + i - dxa;
                        bool ok = rows_ok && xa >= 0 && xa < p.w && xb >= 0 && xb < p.w;
                        const int L2 = p.ctb_log2, cx = (x + i) >> L2, cy = y >> L2;
                        ok = ok && !(nox & (nox_bit((xa >> L2) - cx, ((y + dya) >> L2) - cy) | nox_bit((xb >> L2) - cx, ((y - dya) >> L2) - cy)));
                        const int (&ra)[10] = vertical ? up[k] : mid[k];
                        const int (&rb)[10] = vertical ? dn[k] : mid[k];
                        const int na = dxa < 0 ? ra[i] : (dxa == 0 ? ra[1 + i] : ra[2 + i]);
                        const int nb = dxa < 0 ? rb[2 + i] : (dxa == 0 ? rb[1 + i] : rb[i]);
                        const int e = 2 + sgn(rec - na) + sgn(rec - nb);
                        off = e == 0 ? c.offset[0] : (e == 1 ? c.offset[1] : (e == 3 ? c.offset[2] : (e == 4 ? c.offset[3] : 0)));
                        if (!ok) off = 0;
                    }
                    const int v = rec + off;
                    o[k][i] = copy ? rec : (v < 0 ? 0 : (v > p.max_v ? p.max_v : v));
                }
            }
            st(p.dst + (long long)y * p.pitch, o);
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < 2; k++) {
#if defined(__HIPCC__)
#pragma unroll
#endif
                for (int i = 0; i < 10; i++) { up[k][i] = mid[k][i]; mid[k][i] = dn[k][i]; }
            }
        }
    }
}

} /* namespace saosp */
