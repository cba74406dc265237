/* deblock_sl_packed.h -- the packed kernels' per-segment operands with per-slice offsets (deblock_sl.h): h265_seg_params /
 * h265_seg_rows of deblock_packed_h265.h with one (tc, beta) offset pair per segment instead of the launch's one pair.  Only the
 * two indices of Table 8-12 move, so the filter arithmetic behind them is the QP-map kernels' own. */
#pragma once
#include "deblock_packed_h265.h"
#include "deblock_sl.h"

namespace dbk {

template <bool CHROMA, int CF = 1>
DBK_HD void h265_seg_params_sl(const int (&entry)[4], const int (&qpl)[4], const H265Prm &p, const int (&tc_off)[4],
                               const int (&beta_off)[4], H265Seg &s)
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int bs = entry[i] & kH265BsMask;
        s.entry[i] = entry[i];
        if constexpr (CHROMA) {
            s.beta[i] = 0;
            s.tc[i] = h265_tc(clampi(h265_chroma_qp_cf<CF>(qpl[i] + p.c_qp_offset) + 2 + tc_off[i], 0, 53)) << p.shift;
        } else {
            s.beta[i] = h265_beta(clampi(qpl[i] + beta_off[i], 0, 51)) << p.shift;
            s.tc[i] = h265_tc(clampi(qpl[i] + 2 * (bs - 1) + tc_off[i], 0, 53)) << p.shift;
        }
    }
}

/* TAB form, luma: the table rows of the four segments */
DBK_HD void h265_seg_rows_sl(const int (&entry)[4], const int (&qpl)[4], const H265Prm &p, const DBK_LDS uint32_t *tab,
                             const int (&tc_off)[4], const int (&beta_off)[4], H265Seg &s)
{
    s.tab = tab;
    s.shift = p.shift;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int bs = entry[i] & kH265BsMask;
        s.entry[i] = entry[i];
        s.ib[i] = clampi(qpl[i] + beta_off[i], 0, 51);
        s.it[i] = clampi(qpl[i] + 2 * (bs - 1) + tc_off[i], 0, 53);
        s.tc[i] = 0;
        s.beta[i] = 0;
    }
}

} /* namespace dbk */
