/*
 * deblock_sp.h -- semi-planar chroma (one plane of interleaved Cb / Cr pairs: the NV12 layout and its 16-bit sibling; the _sp
 * entries of the C ABI): the row pieces of an offset block of sample PAIRS taken apart into the two components' row pieces, in the
 * register layouts the packed block procedures work on, and put together again.
 *
 * 8-bit samples (deblock_packed_h265.h: L = columns 0..3, R = columns 4..7 of a row as one dword each).  A row of the block is 16
 * bytes, four dwords d0..d3 = Cb0 Cr0 Cb1 Cr1 | Cb2 Cr2 Cb3 Cr3 | Cb4 .. | Cb6 .. Cr7: the even bytes of (d0, d1) are Cb's L, the
 * odd bytes Cr's L, likewise (d2, d3) and R -- four v_perm_b32 on the way in and four on the way out.
 *
 * 16-bit containers (deblock_packed16.h: W[j] = columns (2j, 2j + 1) of a row as two uint16).  A row is 32 bytes, eight dwords
 * d[i] = (Cb_i, Cr_i): the low halves of (d[2j], d[2j + 1]) are Cb's W[j], the high halves Cr's -- the same on halves of dwords.
 *
 * DBK_HD like deblock_packed.h: tests/sp_sim runs these and the block procedures on the CPU against tests/sp_ref.py.
 */
#pragma once
#include "deblock_packed.h"

namespace dbk {

/* d[0..3] -> (L, R) of component C (0 = the even samples, Cb in NV12 order; 1 = the odd ones) */
template <int C>
DBK_HD void sp_split8(const uint32_t (&d)[4], uint32_t &l, uint32_t &r)
{
    constexpr uint32_t sel = C == 0 ? 0x06040200u : 0x07050301u;
    l = perm(d[1], d[0], sel);
    r = perm(d[3], d[2], sel);
}
/* the (L, R) pairs of both components -> d[0..3] */
DBK_HD void sp_merge8(uint32_t l0, uint32_t r0, uint32_t l1, uint32_t r1, uint32_t (&d)[4])
{
    d[0] = perm(l1, l0, 0x05010400u);
    d[1] = perm(l1, l0, 0x07030602u);
    d[2] = perm(r1, r0, 0x05010400u);
    d[3] = perm(r1, r0, 0x07030602u);
}

/* d[0..7] -> W[0..3] of component C */
template <int C>
DBK_HD void sp_split16(const uint32_t (&d)[8], uint32_t (&w)[4])
{
    constexpr uint32_t sel = C == 0 ? 0x05040100u : 0x07060302u;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) w[j] = perm(d[2 * j + 1], d[2 * j], sel);
}
/* W[0..3] of both components -> d[0..7] */
DBK_HD void sp_merge16(const uint32_t (&w0)[4], const uint32_t (&w1)[4], uint32_t (&d)[8])
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 4; j++) {
        d[2 * j] = perm(w1[j], w0[j], 0x05040100u);
        d[2 * j + 1] = perm(w1[j], w0[j], 0x07060302u);
    }
}

} /* namespace dbk */
