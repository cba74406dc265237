/*
 * sl_sim.cpp -- runs the KERNELS' per-block procedure with per-slice deblocking offsets (gpu_video_codec_amd/csrc: deblock_sl.h,
 * the rule and the 32-bit kernel's form; deblock_sl_packed.h, the packed and fused kernels' per-segment operands) on the CPU over
 * a whole plane, with the kernels' zero padding and bS guards.  TEST-ONLY: built by tests/test_slice_offsets_cpu.py, never part
 * of the product library.
 */
#include <cstdint>

#include "../../gpu_video_codec_amd/csrc/deblock_core.h"
#include "../../gpu_video_codec_amd/csrc/deblock_h265.h"
#define DBK_HOST_SIM 1
#include "../../gpu_video_codec_amd/csrc/deblock_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed_h265.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed16.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl_packed.h"

template <typename T>
static void load_block(const T *plane, long pitch_s, int w, int h, int bx, int by, int (&v)[8][8])
{
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++) {
            const int x = bx * 8 - 4 + c, y = by * 8 - 4 + r;
            v[r][c] = (x >= 0 && x < w && y >= 0 && y < h) ? plane[(long)y * pitch_s + x] : 0;
        }
}
template <typename T>
static void store_block(T *plane, long pitch_s, int w, int h, int bx, int by, const int (&v)[8][8])
{
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++) {
            const int x = bx * 8 - 4 + c, y = by * 8 - 4 + r;
            if (x >= 0 && x < w && y >= 0 && y < h) plane[(long)y * pitch_s + x] = (T)v[r][c];
        }
}

/* CF 0 = luma, 1..3 = a chroma plane of that format; packed 0 = the 32-bit kernel's form, 1 = the packed kernels' per-lane values
 * (h265_seg_params_sl), 2 = luma only: their operand-table rows (h265_seg_rows_sl) */
template <typename T, int CF>
static void run(T *plane, int w, int h, long pitch_s, const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride,
                int unit_log2, const dbk::H265Prm &prm, const int8_t *offs, int offs_stride, int ctb_log2, int packed)
{
    constexpr int sx = CF == 0 ? 1 : dbk::ChromaFmt<CF == 0 ? 1 : CF>::sx, sy = CF == 0 ? 1 : dbk::ChromaFmt<CF == 0 ? 1 : CF>::sy;
    constexpr bool chroma = CF != 0;
    const int nbx = w / 8 + 1, nby = h / 8 + 1;
    uint32_t ktab[dbk::kKTabDwords];
    dbk::ktab_build<true>(ktab, 0, 1, [&](int i) { return dbk::h265_beta(i < 52 ? i : 51) << prm.shift; },
                          [&](int i) { return dbk::h265_tc(i) << prm.shift; });
    auto pair = [&](int cx, int cy) {
        const int8_t *p = offs + 2 * ((long)cy * offs_stride + cx);
        return (unsigned)(uint8_t)p[0] | ((unsigned)(uint8_t)p[1] << 8);
    };
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            int v[8][8], entry[4], qpl[4], cx[2], cy[2], tc_off[4], beta_off[4];
            load_block(plane, pitch_s, w, h, bx, by, v);
            dbk::load_block_bs_h265(vbs4, hbs4, bx, by, nbx, nby, w / 8 + 1, w / 4, entry);
            dbk::h265_block_qpl_xy(map, map_stride, unit_log2, sx, sy, w * sx, h * sy, bx * 8 - 4, by * 8 - 4, qp, qpl);
            dbk::h265_sl_ctbs<sx, sy>(bx, by, w * sx, h * sy, ctb_log2, cx, cy);
            dbk::h265_sl_seg_offs(pair(cx[1], cy[0]), pair(cx[0], cy[1]), pair(cx[1], cy[1]), tc_off, beta_off);
            if (!packed) {
                dbk::filter_block_h265_sl<CF>(v, entry, qpl, prm, tc_off, beta_off);
            } else {
                dbk::H265Seg sg;
                if (packed == 2) dbk::h265_seg_rows_sl(entry, qpl, prm, ktab, tc_off, beta_off, sg);
                else dbk::h265_seg_params_sl<chroma, chroma ? CF : 1>(entry, qpl, prm, tc_off, beta_off, sg);
                if (sizeof(T) == 2) {
                    uint32_t W[8][4];
                    for (int r = 0; r < 8; r++)
                        for (int j = 0; j < 4; j++) W[r][j] = (uint32_t)v[r][2 * j] | ((uint32_t)v[r][2 * j + 1] << 16);
                    if (chroma) dbk::packed_filter_block16_h265<chroma>(W, sg, prm.max_v);
                    else if (packed == 2 && prm.max_v > 2047) dbk::packed_filter_block16_h265<false, true, true>(W, sg, prm.max_v);
                    else if (packed == 2) dbk::packed_filter_block16_h265<false, false, true>(W, sg, prm.max_v);
                    else if (prm.max_v > 2047) dbk::packed_filter_block16_h265<false, true>(W, sg, prm.max_v);
                    else dbk::packed_filter_block16_h265<false>(W, sg, prm.max_v);
                    for (int r = 0; r < 8; r++)
                        for (int j = 0; j < 4; j++) {
                            v[r][2 * j] = W[r][j] & 0xffff;
                            v[r][2 * j + 1] = W[r][j] >> 16;
                        }
                } else {
                    uint32_t L[8], R[8];
                    for (int r = 0; r < 8; r++) {
                        L[r] = (uint32_t)v[r][0] | ((uint32_t)v[r][1] << 8) | ((uint32_t)v[r][2] << 16) | ((uint32_t)v[r][3] << 24);
                        R[r] = (uint32_t)v[r][4] | ((uint32_t)v[r][5] << 8) | ((uint32_t)v[r][6] << 16) | ((uint32_t)v[r][7] << 24);
                    }
                    if (packed == 2) dbk::packed_filter_block_h265<false, true>(L, R, sg);
                    else dbk::packed_filter_block_h265<chroma>(L, R, sg);
                    for (int r = 0; r < 8; r++)
                        for (int c = 0; c < 4; c++) {
                            v[r][c] = (L[r] >> (8 * c)) & 0xff;
                            v[r][4 + c] = (R[r] >> (8 * c)) & 0xff;
                        }
                }
            }
            store_block(plane, pitch_s, w, h, bx, by, v);
        }
}

template <typename T>
static int run_cf(int cf, T *plane, int w, int h, long pitch_s, const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map,
                  int map_stride, int unit_log2, const dbk::H265Prm &prm, const int8_t *offs, int offs_stride, int ctb_log2, int packed)
{
    if (packed == 2 && cf != 0) return 1;
    if (cf == 0) run<T, 0>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else if (cf == 1) run<T, 1>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else if (cf == 2) run<T, 2>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else if (cf == 3) run<T, 3>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else return 1;
    return 0;
}

/* plane_kind: 0 = luma, 1..3 = a chroma plane of a picture of that chroma_format_idc */
extern "C" int sl_sim_filter_plane(void *plane, int w, int h, long pitch_bytes, int sample_bytes, int bit_depth, int plane_kind,
                                   const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride, int unit_log2,
                                   int c_qp_offset, const int8_t *offs, int offs_stride, int ctb_log2, int packed)
{
    const dbk::H265Prm prm = {0, 0, c_qp_offset, bit_depth - 8, (1 << bit_depth) - 1};
    qp = qp > 51 ? 51 : qp;
    if (sample_bytes == 1)
        return run_cf(plane_kind, (uint8_t *)plane, w, h, pitch_bytes, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride,
                      ctb_log2, packed);
    return run_cf(plane_kind, (uint16_t *)plane, w, h, pitch_bytes / 2, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride,
                  ctb_log2, packed);
}
