/*
 * launch_select.h -- what the kernel launchers (the dbk_launch_* functions of the .hip files) share: turning run-time operands into
 * template arguments, the renumbered 1-D grid, the generic kernels' geometry and the small guards every launcher starts with.
 * Internal to the .hip files; not installed.
 *
 * A launcher computes its predicates once as named const values, folds away the operands its kernels do not distinguish, and names
 * each kernel template once inside nested with_bool / with_int calls.  Combinations that exist as no kernel are excluded with
 * `if constexpr` in the innermost body, so that no kernel is instantiated that is never launched.
 */
#ifndef HEVCDBK_LAUNCH_SELECT_H
#define HEVCDBK_LAUNCH_SELECT_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "deblock_kernels.h"

namespace dbksel {

/* f(std::integral_constant<bool, v>) */
template <typename F>
inline void with_bool(bool v, F &&f)
{
    if (v) f(std::true_type{});
    else f(std::false_type{});
}

/* f(std::integral_constant<int, v>) for v out of the list; any other value takes the list's last entry, as the last `else` of a ladder
 * does (the launchers refuse values outside their list before they select) */
template <int V0, int... Vs, typename F>
inline void with_int(int v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
    else if (v == V0) f(std::integral_constant<int, V0>{});
    else with_int<Vs...>(v, f);
}

/* the sample type of with_int<1, 2>(sample_bytes, ...) */
template <int SB>
using sample_t = std::conditional_t<SB == 1, uint8_t, uint16_t>;

/* ---- the renumbered 1-D grid: tiles (fused kernels) or strips (SAO) of all frames as one range of workgroups, split into eight
 * contiguous parts, one per XCD.  The kernels recover (frame, row, column) by exact reciprocal division, which needs dividend <
 * 2^32 / divisor: `exact` says whether that holds.  The fused launchers are behind dbk_deblock_sao[_sp]_supports, which asks no less,
 * and take the grid as it is; the SAO launchers fall back to their 3-D grid when it does not hold.  The grid is 8 * per_xcd
 * workgroups with per_xcd = ceil(total / 8): "the total rounded up to a multiple of 8" and "eight times the rounded-up eighth" are
 * one number.  It is computed from the 64-bit total; a total that does not fit 32 bits (where rounding g.total would give another
 * grid) never arrives: the supports functions bound it for the fused launchers, `exact` for the SAO ones. ---- */
struct RenumberedGrid {
    DbkFusedGrid g;
    unsigned wgs; /* the launch's grid size */
    bool exact;
};
inline RenumberedGrid renumbered_grid(unsigned long long tx, unsigned long long ty, unsigned long long n_frames)
{
    const unsigned long long tpf = tx * ty, total = tpf * n_frames;
    RenumberedGrid r;
    r.exact = total + 8 < (1ull << 31) && (total + 8) * tpf < (1ull << 32) && tpf * tx < (1ull << 32);
    r.g.tiles_x = (uint32_t)tx;
    r.g.tiles_per_frame = (uint32_t)tpf;
    r.g.total = (uint32_t)total;
    r.g.magic_tpf = tpf <= 1 ? 0u : (uint32_t)((1ull << 32) / tpf + 1ull);
    r.g.magic_tx = tx <= 1 ? 0u : (uint32_t)((1ull << 32) / tx + 1ull);
    r.g.per_xcd = (uint32_t)((total + 7) / 8);
    r.wgs = r.g.per_xcd * 8u;
    return r;
}

/* ---- SAO: one workgroup = a strip of `waves` 64 x 64 regions side by side.  The renumbered grid where it is exact (and `renumber`
 * allows it), the plain 3-D grid and a zeroed DbkFusedGrid otherwise ---- */
struct SaoGrid {
    dim3 grid, block;
    DbkFusedGrid g;
    bool swz;
};
inline RenumberedGrid sao_strips(const DbkSaoArgs &a, int waves)
{
    return renumbered_grid((unsigned long long)((a.plane_w + 64 * waves - 1) / (64 * waves)), (unsigned long long)((a.plane_h + 63) / 64),
                           (unsigned long long)a.n_frames);
}
inline SaoGrid sao_grid(const DbkSaoArgs &a, int waves = 4, bool renumber = true)
{
    const RenumberedGrid r = sao_strips(a, waves);
    SaoGrid s;
    s.block = dim3(64 * waves, 1, 1);
    s.swz = renumber && r.exact;
    s.g = s.swz ? r.g : DbkFusedGrid{};
    s.grid = s.swz ? dim3(r.wgs, 1, 1) : dim3((a.plane_w + 64 * waves - 1) / (64 * waves), (a.plane_h + 63) / 64, a.n_frames);
    return s;
}

/* ---- the generic kernels (one lane = one 8x8 block, 64 x 4 blocks per workgroup, blockIdx.z = frame) ---- */
inline dim3 generic_block() { return dim3(64, 4, 1); }
inline dim3 generic_grid(const DbkArgs &a) { return dim3((a.nbx + 63) / 64, (a.nby + 3) / 4, a.n_frames); }

/* ---- guards ---- */
inline bool nothing_to_do(const DbkArgs &a) { return a.n_frames <= 0 || a.nbx <= 0 || a.nby <= 0; }
inline bool nothing_to_do(const DbkSaoArgs &a) { return a.n_frames <= 0 || a.plane_w <= 0 || a.plane_h <= 0; }
/* chroma_format_idc of a picture with chroma planes */
inline bool chroma_format_ok(int chroma_format) { return chroma_format >= 1 && chroma_format <= 3; }

/* block size and dynamic LDS of a launch */
struct LaunchShape {
    unsigned threads;
    unsigned lds;
};

} /* namespace dbksel */

#endif
