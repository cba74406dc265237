/*
 * sao.hip -- sample adaptive offset (ITU-T H.265 clause 8.7.3), the in-loop stage after deblocking.
 * Not present in the reference.  One lane = one 8x8 block of samples, a wave = one 64x64 region; src -> dst
 * because the edge classifier must see deblocked, not offset, neighbours.  The halo (one row above and below, one sample
 * left and right) comes from L1/L2: each sample is fetched from HBM once per pass.
 */
#include <hip/hip_runtime.h>

#include "deblock_kernels.h"
#include "launch_select.h"
#include "sao_packed.h"

namespace {

template <typename T>
struct Q4;
template <>
struct Q4<uint8_t> {
    using W = uint32_t;
    static __device__ __forceinline__ void unpack(W w, int (&o)[4]) { o[0] = w & 0xff; o[1] = (w >> 8) & 0xff; o[2] = (w >> 16) & 0xff; o[3] = w >> 24; }
    static __device__ __forceinline__ W pack(const int (&o)[4]) { return (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24); }
};
template <>
struct Q4<uint16_t> {
    using W = uint2;
    static __device__ __forceinline__ void unpack(W w, int (&o)[4]) { o[0] = w.x & 0xffff; o[1] = w.x >> 16; o[2] = w.y & 0xffff; o[3] = w.y >> 16; }
    static __device__ __forceinline__ W pack(const int (&o)[4]) { return make_uint2((uint32_t)o[0] | ((uint32_t)o[1] << 16), (uint32_t)o[2] | ((uint32_t)o[3] << 16)); }
};

/* samples x-1 .. x+8 of one row (x a multiple of 8) into o[0..9]; positions outside the row hold junk the caller never uses */
template <typename T>
__device__ __forceinline__ void load10(const uint8_t *row, int x, int w, int (&o)[10])
{
    using W = typename Q4<T>::W;
    int c0[4], c1[4], l[4], r[4];
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)x * sizeof(T)), c0);
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x + 4) * sizeof(T)), c1);
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x >= 4 ? x - 4 : 0) * sizeof(T)), l);
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x + 12 <= w ? x + 8 : w - 4) * sizeof(T)), r);
    o[0] = l[3];
#pragma unroll
    for (int i = 0; i < 4; i++) { o[1 + i] = c0[i]; o[5 + i] = c1[i]; }
    o[9] = r[0];
}
template <typename T>
__device__ __forceinline__ void load8(const uint8_t *row, int x, int (&o)[8])
{
    using W = typename Q4<T>::W;
    int c0[4], c1[4];
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)x * sizeof(T)), c0);
    Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x + 4) * sizeof(T)), c1);
#pragma unroll
    for (int i = 0; i < 4; i++) { o[i] = c0[i]; o[4 + i] = c1[i]; }
}
template <typename T>
__device__ __forceinline__ void store8(uint8_t *row, int x, const int (&o)[8])
{
    using W = typename Q4<T>::W;
    const int a[4] = {o[0], o[1], o[2], o[3]}, b[4] = {o[4], o[5], o[6], o[7]};
    *reinterpret_cast<W *>(row + (size_t)x * sizeof(T)) = Q4<T>::pack(a);
    *reinterpret_cast<W *>(row + (size_t)(x + 4) * sizeof(T)) = Q4<T>::pack(b);
}

__device__ __forceinline__ int sgn(int v) { return (v > 0) - (v < 0); }

/*
 * Workgroup -> (256 x 64 strip, frame).  SWZ: a 1-D grid whose workgroups are renumbered so that each XCD (workgroups are
 * dealt to the 8 XCDs round-robin -- an observation used for speed only) works through a CONTIGUOUS range of strips,
 * row-major inside a frame.  The halo of an edge-offset CTB -- the 16-byte row loads reach 4 bytes into the strip to the
 * left and right, the three-row window one row into the strips above and below -- then lies in lines a neighbouring
 * workgroup of the SAME XCD fetches as well, i.e. in that XCD's L2, instead of being fetched from HBM once per XCD
 * (round 2: 1.48 x the plane's bytes read for one third edge CTBs; the same renumbering took the fused deblocking + SAO
 * kernel from 2.0 x to 1.004 x).  Grids too large for the exact 32-bit reciprocal divisions keep the 3-D numbering.
 */
template <bool SWZ>
__device__ __forceinline__ bool sao_strip(const DbkFusedGrid &g, int &wx, int &wy, int &f)
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

/*
 * One lane = one 8x8 block of samples (the unit of the keep map; inside one CTB since CTBs are at least 8 samples): the
 * CTB parameters and the keep flag are fetched once, and the edge classifier slides a three-row window down the block, so a
 * row is loaded once per lane (10 rows for 8 rows of output) instead of three times per output row.
 */
/* the CTB bit that speaks for the neighbouring CTB (dcx, dcy), each -1 / 0 / 1; (0, 0) = the CTB itself: nothing */
__device__ __forceinline__ uint32_t sao_nox_bit(int dcx, int dcy)
{
    using namespace saonox;
    return dcy < 0 ? (dcx < 0 ? UL : (dcx > 0 ? UR : U)) : (dcy > 0 ? (dcx < 0 ? DL : (dcx > 0 ? DR : D)) : (dcx < 0 ? L : (dcx > 0 ? R : 0u)));
}


/* One block of the _g4 kernels (planes whose sizes are multiples of 4, not 8): 8 or 4 columns by 8 or 4 rows at (x, y0), the short
 * ones being the last of their row / column of blocks.  The per-sample procedure of sao_kernel_body.inc with every position tested
 * against the picture (a neighbour outside plane_w x plane_h: no offset, 8.7.3.2) and against the CTB's boundary byte `nox`
 * (0 = nothing forbidden); a narrow block moves 4 samples per row -- nothing beyond plane_w is read or written -- a short one 4 rows */
template <typename T>
__device__ __forceinline__ void sao_block_g4(const DbkSaoArgs &a, uint32_t nox, const uint8_t *src, uint8_t *dst, int x, int y0,
                                             const DbkSaoCtb &c, bool kept)
{
    using W = typename Q4<T>::W;
    const bool w8 = x + 8 <= a.plane_w;
    const int nr = y0 + 8 <= a.plane_h ? 8 : 4;
    auto ld8 = [&](const uint8_t *row, int (&o)[8]) {
        int c0[4], c1[4];
        Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)x * sizeof(T)), c0);
        Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(w8 ? x + 4 : x) * sizeof(T)), c1); /* narrow: never used */
#pragma unroll
        for (int i = 0; i < 4; i++) { o[i] = c0[i]; o[4 + i] = c1[i]; }
    };
    auto st8 = [&](uint8_t *row, const int (&o)[8]) {
        const int lo[4] = {o[0], o[1], o[2], o[3]}, hi[4] = {o[4], o[5], o[6], o[7]};
        *reinterpret_cast<W *>(row + (size_t)x * sizeof(T)) = Q4<T>::pack(lo);
        if (w8) *reinterpret_cast<W *>(row + (size_t)(x + 4) * sizeof(T)) = Q4<T>::pack(hi);
    };
    if (kept || c.type == 0 || c.type > 2) {
#pragma unroll
        for (int r = 0; r < 8; r++)
            if (r < nr) {
                int o[8];
                ld8(src + (long long)(y0 + r) * a.pitch, o);
                st8(dst + (long long)(y0 + r) * a.pitch, o);
            }
        return;
    }
    if (c.type == 1) { /* band offset: bandTable[(k + sao_band_position) & 31] = k + 1 */
#pragma unroll
        for (int r = 0; r < 8; r++)
            if (r < nr) {
                int o[8];
                ld8(src + (long long)(y0 + r) * a.pitch, o);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int k = ((o[i] >> a.band_shift) - (int)c.cls) & 31;
                    const int off = k == 0 ? c.offset[0] : (k == 1 ? c.offset[1] : (k == 2 ? c.offset[2] : (k == 3 ? c.offset[3] : 0)));
                    const int v = o[i] + off;
                    o[i] = v < 0 ? 0 : (v > a.max_v ? a.max_v : v);
                }
                st8(dst + (long long)(y0 + r) * a.pitch, o);
            }
        return;
    }
    /* edge offset, Table 8-13: class 0 (-1,0)/(1,0); 1 (0,-1)/(0,1); 2 (-1,-1)/(1,1); 3 (1,-1)/(-1,1) */
    const int cls = c.cls & 3;
    const int dxa = cls == 1 ? 0 : (cls == 3 ? 1 : -1);
    const bool vertical = cls != 0;
    const int dya = vertical ? -1 : 0;
    auto row_at = [&](int y) { return src + (long long)(y < 0 ? 0 : (y >= a.plane_h ? a.plane_h - 1 : y)) * a.pitch; };
    /* samples x-1 .. x+8 of a row; positions outside the row hold junk that no sample inside the picture uses */
    auto ld10 = [&](const uint8_t *row, int (&o)[10]) {
        int m[8], l[4], r[4];
        ld8(row, m);
        Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x >= 4 ? x - 4 : 0) * sizeof(T)), l);
        Q4<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x + 12 <= a.plane_w ? x + 8 : a.plane_w - 4) * sizeof(T)), r);
        o[0] = l[3];
#pragma unroll
        for (int i = 0; i < 8; i++) o[1 + i] = m[i];
        o[9] = r[0];
    };
    int up[10], mid[10], dn[10];
    ld10(row_at(y0 - 1), up);
    ld10(row_at(y0), mid);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        if (r < nr) {
            const int y = y0 + r;
            ld10(row_at(y + 1), dn);
            const bool rows_ok = !vertical || (y > 0 && y < a.plane_h - 1);
            int o[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int rec = mid[1 + i];
                const int xa = x + i + dxa, xb = x + i - dxa;
                bool ok = rows_ok && xa >= 0 && xa < a.plane_w && xb >= 0 && xb < a.plane_w;
                const int L2 = a.ctb_log2, cx = (x + i) >> L2, cy = y >> L2; /* per sample: the CTB either neighbour lies in, against the byte */
                ok = ok && !(nox & (sao_nox_bit((xa >> L2) - cx, ((y + dya) >> L2) - cy) | sao_nox_bit((xb >> L2) - cx, ((y - dya) >> L2) - cy)));
                const int (&ra)[10] = vertical ? up : mid;
                const int (&rb)[10] = vertical ? dn : mid;
                const int na = dxa < 0 ? ra[i] : (dxa == 0 ? ra[1 + i] : ra[2 + i]);
                const int nb = dxa < 0 ? rb[2 + i] : (dxa == 0 ? rb[1 + i] : rb[i]);
                const int e = 2 + sgn(rec - na) + sgn(rec - nb);
                const int off = e == 0 ? c.offset[0] : (e == 1 ? c.offset[1] : (e == 3 ? c.offset[2] : (e == 4 ? c.offset[3] : 0)));
                const int v = rec + (ok ? off : 0);
                o[i] = v < 0 ? 0 : (v > a.max_v ? a.max_v : v);
            }
            st8(dst + (long long)y * a.pitch, o);
#pragma unroll
            for (int i = 0; i < 10; i++) { up[i] = mid[i]; mid[i] = dn[i]; }
        }
    }
}

/* PK16: 16-bit containers up to 12 bit take the packed block procedure in waves off the border.  The body is written once
 * (sao_kernel_body.inc) for the kernel and its _nox twin */
template <typename T, bool SWZ, bool PK16 = false>
__global__ __launch_bounds__(256) void sao_kernel(const DbkSaoArgs a, const DbkFusedGrid g)
{
    constexpr bool NOX = false;
    [[maybe_unused]] constexpr bool G4 = false;
    [[maybe_unused]] const DbkSaoNox nx = {};
#include "sao_kernel_body.inc"
}
template <typename T, bool SWZ, bool PK16 = false>
__global__ __launch_bounds__(256) void sao_nox_kernel(const DbkSaoArgs a, const DbkFusedGrid g, const DbkSaoNox nx)
{
    constexpr bool NOX = true;
    [[maybe_unused]] constexpr bool G4 = false;
#include "sao_kernel_body.inc"
}
/* planes whose sizes are multiples of 4, not 8 (the _g4 entries): the _nox twin's twin; nx.nox may be NULL */
template <typename T, bool SWZ, bool PK16 = false>
__global__ __launch_bounds__(256) void sao_g4_kernel(const DbkSaoArgs a, const DbkFusedGrid g, const DbkSaoNox nx)
{
    constexpr bool NOX = true;
    [[maybe_unused]] constexpr bool G4 = true;
#include "sao_kernel_body.inc"
}

/* ------------------------------------------------------------------------------------------ */
/* 8-bit samples: packed-int16 arithmetic, table look-ups by v_perm_b32                         */
/*
 * Same mapping (one lane = one 8x8 block, a wave = one 64x64 region, so with 64-sample CTBs a wave runs ONE path) and the
 * same sliding three-row window, but two samples per VGPR and no per-sample selects:
 *   - a row's 8 samples are four int16 pairs E0 = (s0, s2), O0 = (s1, s3), E1 = (s4, s6), O1 = (s5, s7), one v_perm_b32
 *     each from the row's two dwords; the same instruction, fed the halo dword, makes the pairs shifted one sample left
 *     (lE0, lE1; the left neighbours of O0 / O1 are E0 / E1 themselves) and right (rO0, rO1): every neighbour pair of
 *     Table 8-13 is one of these eight registers of the row above, the row itself or the row below;
 *   - sign(rec - a) + sign(rec - b) + 2 = clamp(rec + 1 - a, 0, 2) + clamp(rec + 1 - b, 0, 2) in both halves at once;
 *   - that index (0..4), or min(bandIdx, 4) for the band offset, selects one of five offset bytes through v_perm_b32 (the
 *     bytes are biased by 128 so that they are plain unsigned bytes; the bias rides on rec);
 *   - picture-border samples (a neighbour outside the picture: no offset) force the index to "none" in the lanes / rows
 *     concerned, compiled only into the instantiation for waves that touch the border.
 * About 9 VALU instructions per sample instead of ~20.
 */
using sao8::SaoRow;
using sao8::SaoRaw;
using sao8::spk;
using sao8::supk;
using sao8::s_pk;
using sao8::s_splat;

typedef uint32_t sao_u32x4 __attribute__((ext_vector_type(4), aligned(4))); /* 16 bytes at a 4-byte-aligned address */
typedef uint32_t sao_u32x2b __attribute__((ext_vector_type(2)));             /* operands of the raw buffer builtins */
typedef uint32_t sao_u32x4b __attribute__((ext_vector_type(4)));

/* HALO: the neighbours to the left / right take part.  INNER (wave-uniform): every lane's 16 bytes x-4 .. x+11 lie inside
 * the row, so the row is ONE 16-byte load per lane; otherwise three loads with the halo positions moved inside the row */
template <bool HALO, bool INNER>
__device__ __forceinline__ SaoRow sao_load_row(const uint8_t *row, int x, int w)
{
    SaoRaw q;
    q.lh = q.rh = 0u;
    if constexpr (HALO && INNER) {
        const sao_u32x4 v = *reinterpret_cast<const sao_u32x4 *>(row + x - 4);
        q.lh = v.x; q.cx = v.y; q.cy = v.z; q.rh = v.w;
    } else {
        const uint2 c = *reinterpret_cast<const uint2 *>(row + x);
        q.cx = c.x; q.cy = c.y;
        if constexpr (HALO) {
            /* positions outside the row read a valid dword of the row instead; the border masks discard what comes of it */
            q.lh = *reinterpret_cast<const uint32_t *>(row + (x >= 4 ? x - 4 : 0));
            q.rh = *reinterpret_cast<const uint32_t *>(row + (x + 12 <= w ? x + 8 : w - 4));
        }
    }
    return sao8::unpack<HALO>(q);
}

__device__ __forceinline__ uint32_t sao_apply(uint32_t rec, uint32_t idx, uint32_t tab_lo, uint32_t tab_hi)
{
    return sao8::apply(rec, idx, tab_lo, tab_hi);
}
__device__ __forceinline__ uint32_t sao_edge_idx(uint32_t rec, uint32_t a, uint32_t b) { return sao8::edge_idx(rec, a, b); }

template <int BORDER> /* 0 = off the border; 1 = the picture border from x, y0; 2 = the block's mask m (saonox::block_mask) */
__device__ __forceinline__ void sao8_edge_block(const DbkSaoArgs &a, const uint8_t *src, uint8_t *dst, int x, int y0, int cls,
                                                uint32_t tab_lo, uint32_t tab_hi, uint32_t m = 0u)
{
    auto row_at = [&](int y) { return src + (long long)(y < 0 ? 0 : (y >= a.plane_h ? a.plane_h - 1 : y)) * a.pitch; };
    const bool horizontal = cls != 1; /* neighbours to the left / right take part: the halo dwords are needed */
    const bool vertical = cls != 0;   /* neighbours in the rows above / below take part */
    SaoRow up, mid, dn;
    if (horizontal) {
        up = sao_load_row<true, BORDER == 0>(row_at(y0 - 1), x, a.plane_w);
        mid = sao_load_row<true, BORDER == 0>(row_at(y0), x, a.plane_w);
    } else {
        up = sao_load_row<false, false>(row_at(y0 - 1), x, a.plane_w);
        mid = sao_load_row<false, false>(row_at(y0), x, a.plane_w);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        dn = horizontal ? sao_load_row<true, BORDER == 0>(row_at(y + 1), x, a.plane_w) : sao_load_row<false, false>(row_at(y + 1), x, a.plane_w);
        uint32_t i0, i1, i2, i3; /* indices of E0, O0, E1, O1 */
        if (cls == 0) {          /* (-1, 0) / (1, 0) */
            i0 = sao_edge_idx(mid.E0, mid.lE0, mid.O0);
            i1 = sao_edge_idx(mid.O0, mid.E0, mid.rO0);
            i2 = sao_edge_idx(mid.E1, mid.lE1, mid.O1);
            i3 = sao_edge_idx(mid.O1, mid.E1, mid.rO1);
        } else if (cls == 1) {   /* (0, -1) / (0, 1) */
            i0 = sao_edge_idx(mid.E0, up.E0, dn.E0);
            i1 = sao_edge_idx(mid.O0, up.O0, dn.O0);
            i2 = sao_edge_idx(mid.E1, up.E1, dn.E1);
            i3 = sao_edge_idx(mid.O1, up.O1, dn.O1);
        } else if (cls == 2) {   /* (-1, -1) / (1, 1) */
            i0 = sao_edge_idx(mid.E0, up.lE0, dn.O0);
            i1 = sao_edge_idx(mid.O0, up.E0, dn.rO0);
            i2 = sao_edge_idx(mid.E1, up.lE1, dn.O1);
            i3 = sao_edge_idx(mid.O1, up.E1, dn.rO1);
        } else {                 /* (1, -1) / (-1, 1) */
            i0 = sao_edge_idx(mid.E0, up.O0, dn.lE0);
            i1 = sao_edge_idx(mid.O0, up.rO0, dn.E0);
            i2 = sao_edge_idx(mid.E1, up.O1, dn.lE1);
            i3 = sao_edge_idx(mid.O1, up.rO1, dn.E1);
        }
        if constexpr (BORDER == 2) { /* a neighbour outside the picture, or across a slice / tile boundary not to be crossed */
            if (cls == 0) saonox::mask_row<0, 8>(m, r, i0, i1, i2, i3);
            else if (cls == 1) saonox::mask_row<1, 8>(m, r, i0, i1, i2, i3);
            else if (cls == 2) saonox::mask_row<2, 8>(m, r, i0, i1, i2, i3);
            else saonox::mask_row<3, 8>(m, r, i0, i1, i2, i3);
        }
        if constexpr (BORDER == 1) { /* a neighbour outside the picture: edgeIdx 0 (8.7.3.2) */
            if (vertical && (y == 0 || y == a.plane_h - 1)) i0 = i1 = i2 = i3 = 0x00020002u | sao8::kSel;
            if (horizontal && x == 0) i0 = (i0 & 0xffff0000u) | 0x0c02u;                       /* sample 0: low half of E0 */
            if (horizontal && x + 8 == a.plane_w) i3 = (i3 & 0x0000ffffu) | 0x0c020000u;  /* sample 7: high half of O1 */
        }
        const uint32_t e0 = sao_apply(mid.E0, i0, tab_lo, tab_hi), o0 = sao_apply(mid.O0, i1, tab_lo, tab_hi);
        const uint32_t e1 = sao_apply(mid.E1, i2, tab_lo, tab_hi), o1 = sao_apply(mid.O1, i3, tab_lo, tab_hi);
        uint2 out;
        out.x = e0 | (o0 << 8);
        out.y = e1 | (o1 << 8);
        *reinterpret_cast<uint2 *>(dst + (long long)y * a.pitch + x) = out;
        up = mid;
        mid = dn;
    }
}

/* the body is written once (sao8_kernel_body.inc) for the kernel and its _nox twin, as for sao_kernel */
template <bool SWZ, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sao8_kernel(const DbkSaoArgs a, const DbkFusedGrid g)
{
    constexpr bool NOX = false;
    [[maybe_unused]] constexpr bool G4 = false;
    [[maybe_unused]] const DbkSaoNox nx = {};
#include "sao8_kernel_body.inc"
}
template <bool SWZ, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sao8_nox_kernel(const DbkSaoArgs a, const DbkFusedGrid g, const DbkSaoNox nx)
{
    constexpr bool NOX = true;
    [[maybe_unused]] constexpr bool G4 = false;
#include "sao8_kernel_body.inc"
}
template <bool SWZ, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void sao8_g4_kernel(const DbkSaoArgs a, const DbkFusedGrid g, const DbkSaoNox nx)
{
    constexpr bool NOX = true;
    [[maybe_unused]] constexpr bool G4 = true;
#include "sao8_kernel_body.inc"
}

/* ---- the launchers.  A kernel comes in three forms, with one body: plain (a, g), the _nox twin (a, g, nx) for calls with boundary
 * bytes, and the _g4 form (a, g, nx; nx.nox may be NULL) for planes whose sizes are multiples of 4, not 8 ---- */
#ifdef HEVCDBK_DIAG
constexpr bool kNarrowStrips = true; /* sao8[_nox]_kernel<true, 1 | 2>: the wg_cap knob */
#else
constexpr bool kNarrowStrips = false;
#endif

template <bool G4, bool NOX, bool SWZ, int WAVES>
void launch_sao8(const dbksel::SaoGrid &sg, hipStream_t stream, const DbkSaoArgs &a, const DbkSaoNox &nx)
{
    if constexpr (G4) hipLaunchKernelGGL((sao8_g4_kernel<SWZ, WAVES>), sg.grid, sg.block, 0, stream, a, sg.g, nx);
    else if constexpr (NOX) hipLaunchKernelGGL((sao8_nox_kernel<SWZ, WAVES>), sg.grid, sg.block, 0, stream, a, sg.g, nx);
    else hipLaunchKernelGGL((sao8_kernel<SWZ, WAVES>), sg.grid, sg.block, 0, stream, a, sg.g);
}

template <bool G4, bool NOX, typename T, bool SWZ, bool PK16>
void launch_sao_t(const dbksel::SaoGrid &sg, hipStream_t stream, const DbkSaoArgs &a, const DbkSaoNox &nx)
{
    if constexpr (G4) hipLaunchKernelGGL((sao_g4_kernel<T, SWZ, PK16>), sg.grid, sg.block, 0, stream, a, sg.g, nx);
    else if constexpr (NOX) hipLaunchKernelGGL((sao_nox_kernel<T, SWZ, PK16>), sg.grid, sg.block, 0, stream, a, sg.g, nx);
    else hipLaunchKernelGGL((sao_kernel<T, SWZ, PK16>), sg.grid, sg.block, 0, stream, a, sg.g);
}

/* G4: the two predicates without their demand for multiples of 8, the _g4 kernels whether or not there are boundary bytes, and
 * none of the diagnostic library's knobs */
template <bool G4>
hipError_t launch_sao(const DbkSaoArgs &a, int sample_bytes, hipStream_t stream, const DbkSaoNox *nxp)
{
    using namespace dbksel;
    if (nothing_to_do(a)) return hipSuccess;
    const bool small = (unsigned long long)a.pitch * (unsigned long long)a.plane_h < (1ull << 31); /* 32-bit buffer offsets */
    const bool mult8 = G4 || (a.plane_w % 8 == 0 && a.plane_h % 8 == 0);
    /* 8-bit planes whose rows and frames are 8-byte aligned take the packed kernel (every lane moves 8 bytes at once) */
    const bool aligned8 = sample_bytes == 1 && a.pitch % 8 == 0 && a.frame_stride % 8 == 0 && ((uintptr_t)a.src % 8) == 0 &&
                          ((uintptr_t)a.dst % 8) == 0 && mult8 && a.max_v == 255 && a.band_shift == 3 && small;
    /* 16-bit containers up to 12 bit (the packed procedure's int16 fields; SaoOffsetVal scaled as the standard does), planes the
     * buffer resources can address: the packed path in every wave off the picture border */
    const bool pk16 = sample_bytes != 1 && a.max_v <= 4095 && a.band_shift >= 3 && (1 << (a.band_shift + 5)) - 1 == a.max_v &&
                      a.pitch % 4 == 0 && a.frame_stride % 4 == 0 && ((uintptr_t)a.src % 4) == 0 && ((uintptr_t)a.dst % 4) == 0 && mult8 &&
                      small;
    int waves = 4; /* 64 x 64 regions (waves) side by side in one workgroup */
    bool renumber = true;
#ifdef HEVCDBK_DIAG
    if constexpr (!G4) {
        renumber = !g_dbk_diag.noswz; /* A/B knob of the diagnostic library: the plain 3-D numbering */
        /* A/B knob: narrower workgroups of the packed 8-bit kernel.  They exist for the renumbered grid only (sao8_kernel<true, 1 | 2>):
         * with the plain 3-D numbering -- the noswz knob, or a grid too large to renumber -- the launch is sao8_kernel<false, 4>, whose
         * strips are 256 samples wide, and block / grid must be sized for that (half or three quarters of each strip row
         * stayed unwritten when both knobs were set) */
        const int knob = g_dbk_diag.wg_cap / 64;
        if (aligned8 && renumber && (g_dbk_diag.wg_cap == 64 || g_dbk_diag.wg_cap == 128) && sao_strips(a, knob).exact) waves = knob;
    }
#endif
    const SaoGrid sg = sao_grid(a, waves, renumber);
    const DbkSaoNox nx = nxp ? *nxp : DbkSaoNox{nullptr, 0, 0}; /* no bytes: no direction is forbidden */
    with_bool(nxp != nullptr, [&](auto HAS_NX) {
        constexpr bool NOX = !G4 && HAS_NX; /* the _g4 kernels take nx either way */
        with_bool(sg.swz, [&](auto SWZ) {
            if (aligned8) {
                with_int<1, 2, 4>(waves, [&](auto WAVES) {
                    if constexpr (WAVES == 4 || (kNarrowStrips && SWZ && !G4)) launch_sao8<G4, NOX, SWZ, WAVES>(sg, stream, a, nx);
                });
            } else if (sample_bytes == 1) {
                launch_sao_t<G4, NOX, uint8_t, SWZ, false>(sg, stream, a, nx);
            } else {
                with_bool(pk16 && SWZ, [&](auto PK16) { /* the packed form reads the renumbered grid */
                    if constexpr (SWZ || !PK16) launch_sao_t<G4, NOX, uint16_t, SWZ, PK16>(sg, stream, a, nx);
                });
            }
        });
    });
    return hipGetLastError();
}

} /* namespace */

hipError_t dbk_launch_sao(const DbkSaoArgs &a, int sample_bytes, hipStream_t stream, const DbkSaoNox *nxp)
{
    return launch_sao<false>(a, sample_bytes, stream, nxp);
}

/* planes whose sizes are multiples of 4 (the _g4 entries): dbk_launch_sao's grid and choice of kernel without its demand for multiples
 * of 8, the _g4 kernels; nxp == NULL: no boundary bytes */
hipError_t dbk_launch_sao_g4(const DbkSaoArgs &a, int sample_bytes, hipStream_t stream, const DbkSaoNox *nxp)
{
    return launch_sao<true>(a, sample_bytes, stream, nxp);
}

/* ---- rectangular CTBs (4:2:2 chroma: CtbSizeY / 2 wide, CtbSizeY tall) ----------------------------------------------------
 * A CTB of (1 << L) x (1 << (L + 1)) samples is two square CTBs of (1 << L) one above the other with the same parameters, so
 * the parameter rows are doubled once per call (a few KiB: one entry per CTB) and the square kernels -- plain SAO and the fused
 * deblocking + SAO kernels, fast paths included -- run unchanged on the result. */
namespace {
__global__ __launch_bounds__(256) void sao_rows_x2_kernel(const DbkSaoCtb *src, int src_stride, long long src_frame_stride,
                                                          DbkSaoCtb *dst, int cols, int rows, long long total)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long per_frame = (long long)rows * cols;
    const long long f = i / per_frame, k = i - f * per_frame;
    const int r = (int)(k / cols), c = (int)(k - (long long)r * cols);
    dst[i] = src[f * src_frame_stride + (long long)(r >> 1) * src_stride + c];
}
} /* namespace */

size_t dbk_sao_rows_x2_entries(const DbkSaoArgs &a)
{
    const long long cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    return (size_t)(cols * rows * (a.params_frame_stride ? a.n_frames : 1));
}

hipError_t dbk_launch_sao_rows_x2(DbkSaoArgs &a, DbkSaoCtb *dst, hipStream_t stream)
{
    const int cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    const long long total = (long long)dbk_sao_rows_x2_entries(a);
    if (total > 0)
        hipLaunchKernelGGL(sao_rows_x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a.params, a.params_stride,
                           a.params_frame_stride, dst, cols, rows, total);
    a.params = dst;
    a.params_stride = cols;
    a.params_frame_stride = a.params_frame_stride ? (long long)rows * cols : 0;
    return hipGetLastError();
}

/* ---- slice / tile boundaries SAO must not look across (H.265 8.7.3.2) ------------------------------------------------------
 * One lane per CTB: for each of the eight neighbouring CTBs inside the picture, the bit is set when that CTB lies in another
 * slice whose order and flags forbid it -- the neighbour's slice earlier in decoding order and THIS slice's
 * slice_loop_filter_across_slices_enabled_flag 0, or later and the NEIGHBOUR's flag 0 -- or in another tile while
 * loop_filter_across_tiles_enabled_flag is 0. */
namespace {
__global__ __launch_bounds__(256) void sao_borders_kernel(const uint16_t *slice_idx, const uint8_t *slice_across, const uint16_t *tile_idx,
                                                          int tiles_across, int ctbs_x, int ctbs_y, int in_stride, uint8_t *nox, int nox_stride)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ctbs_x * ctbs_y) return;
    const int cy = i / ctbs_x, cx = i - cy * ctbs_x;
    const long long at = (long long)cy * in_stride + cx;
    const unsigned s = slice_idx[at], fl = slice_across[at], t = tile_idx ? tile_idx[at] : 0u;
    uint32_t b = 0u;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if ((dx == 0 && dy == 0) || cx + dx < 0 || cx + dx >= ctbs_x || cy + dy < 0 || cy + dy >= ctbs_y) continue;
            const long long n = at + (long long)dy * in_stride + dx;
            const unsigned s2 = slice_idx[n];
            const bool by_slice = (s2 < s && fl == 0u) || (s < s2 && slice_across[n] == 0u);
            const bool by_tile = !tiles_across && tile_idx && tile_idx[n] != t;
            if (by_slice || by_tile) b |= sao_nox_bit(dx, dy);
        }
    nox[(long long)cy * nox_stride + cx] = (uint8_t)b;
}

/* the bytes of CTBs of (1 << L) x (2 << L) samples as those of the square CTBs they are halves of: what lies below the upper half
 * is the CTB itself (D cleared) and, diagonally, the left / right CTB (DL := L, DR := R); the lower half likewise upwards */
__global__ __launch_bounds__(256) void sao_nox_rows_x2_kernel(const uint8_t *src, int src_stride, long long src_frame_stride, uint8_t *dst,
                                                              int cols, int rows, long long total)
{
    using namespace saonox;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const long long per_frame = (long long)rows * cols;
    const long long f = i / per_frame, k = i - f * per_frame;
    const int r = (int)(k / cols), c = (int)(k - (long long)r * cols);
    const uint32_t b = src[f * src_frame_stride + (long long)(r >> 1) * src_stride + c];
    const uint32_t l = (b & L) ? 1u : 0u, rr = (b & R) ? 1u : 0u;
    dst[i] = (uint8_t)((r & 1) ? ((b & ~(U | UL | UR)) | (l ? UL : 0u) | (rr ? UR : 0u)) : ((b & ~(D | DL | DR)) | (l ? DL : 0u) | (rr ? DR : 0u)));
}
} /* namespace */

hipError_t dbk_launch_sao_borders(const uint16_t *slice_idx, const uint8_t *slice_across, const uint16_t *tile_idx, int tiles_across,
                                  int ctbs_x, int ctbs_y, int in_stride, uint8_t *nox, int nox_stride, hipStream_t stream)
{
    const int total = ctbs_x * ctbs_y;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_borders_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, slice_idx, slice_across, tile_idx,
                       tiles_across, ctbs_x, ctbs_y, in_stride, nox, nox_stride);
    return hipGetLastError();
}

hipError_t dbk_launch_sao_nox_rows_x2(const DbkSaoArgs &a, DbkSaoNox &nx, uint8_t *dst, hipStream_t stream)
{
    const int cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    const bool per_frame = nx.frame_stride != 0;
    const long long total = (long long)cols * rows * (per_frame ? a.n_frames : 1);
    if (total > 0)
        hipLaunchKernelGGL(sao_nox_rows_x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, nx.nox, nx.stride,
                           nx.frame_stride, dst, cols, rows, total);
    nx.nox = dst;
    nx.stride = cols;
    nx.frame_stride = per_frame ? (long long)rows * cols : 0;
    return hipGetLastError();
}
