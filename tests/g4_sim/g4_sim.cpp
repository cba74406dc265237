/*
 * g4_sim.cpp -- runs the _g4 KERNELS' per-block procedure (gpu_video_codec_amd/csrc: deblock_h265.h load_block_bs_h265_g4 with the
 * kernels' zero padding, deblock_sl.h for the offsets, the 32-bit form and the packed kernels' per-lane form) on the CPU over a
 * whole chroma plane whose sizes are multiples of 4, not 8.  TEST-ONLY: built by tests/test_g4_cpu.py, never part of the product
 * library.
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

/* the kernels' loads: a half or a row outside the picture is zeros, and "outside" on the right / below is what g4_right_in /
 * g4_below_in say of the block -- NOT a test of every sample against w and h */
template <typename T>
static void load_block(const T *plane, long pitch_s, int w, int h, int bx, int by, int (&v)[8][8])
{
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, w);
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++) {
            const int x = bx * 8 - 4 + c, y = by * 8 - 4 + r;
            v[r][c] = ((c < 4 ? lv : rv) && y >= 0 && y < h) ? plane[(long)y * pitch_s + x] : 0;
        }
}
template <typename T>
static void store_block(T *plane, long pitch_s, int w, int h, int bx, int by, const int (&v)[8][8])
{
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, w);
    for (int r = 0; r < 8; r++)
        for (int c = 0; c < 8; c++) {
            const int x = bx * 8 - 4 + c, y = by * 8 - 4 + r;
            if ((c < 4 ? lv : rv) && y >= 0 && y < h) plane[(long)y * pitch_s + x] = (T)v[r][c];
        }
}

/* CF 1..3 = a chroma plane of that format; packed 0 = the 32-bit kernel's form, 1 = the packed kernels' per-lane values.
 * offs == NULL: no per-slice offsets (every pair reads (0, 0)); prm.tc_off / beta_off are ADDED to the pairs, as the kernels do */
template <typename T, int CF>
static void run(T *plane, int w, int h, long pitch_s, const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride,
                int unit_log2, const dbk::H265Prm &prm0, const int8_t *offs, int offs_stride, int ctb_log2, int packed)
{
    constexpr int sx = dbk::ChromaFmt<CF>::sx, sy = dbk::ChromaFmt<CF>::sy;
    const int nbx = w / 8 + 1, nby = h / 8 + 1;
    dbk::H265Prm prm = prm0;
    prm.tc_off = prm.beta_off = 0;
    auto pair = [&](int cx, int cy) {
        if (!offs) return 0u;
        const int8_t *p = offs + 2 * ((long)cy * offs_stride + cx);
        return (unsigned)(uint8_t)p[0] | ((unsigned)(uint8_t)p[1] << 8);
    };
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            int v[8][8], entry[4], qpl[4], cx[2], cy[2], tc_off[4], beta_off[4];
            load_block(plane, pitch_s, w, h, bx, by, v);
            dbk::load_block_bs_h265_g4(vbs4, hbs4, bx, by, w, h, w / 8 + 1, w / 4, entry);
            dbk::h265_block_qpl_xy(map, map_stride, unit_log2, sx, sy, w * sx, h * sy, bx * 8 - 4, by * 8 - 4, qp, qpl);
            dbk::h265_sl_ctbs<sx, sy>(bx, by, w * sx, h * sy, ctb_log2, cx, cy);
            dbk::h265_sl_seg_offs(pair(cx[1], cy[0]), pair(cx[0], cy[1]), pair(cx[1], cy[1]), tc_off, beta_off);
            for (int s = 0; s < 4; s++) {
                tc_off[s] += prm0.tc_off;
                beta_off[s] += prm0.beta_off;
            }
            if (!packed) {
                dbk::filter_block_h265_sl<CF>(v, entry, qpl, prm, tc_off, beta_off);
            } else {
                dbk::H265Seg sg;
                dbk::h265_seg_params_sl<true, CF>(entry, qpl, prm, tc_off, beta_off, sg);
                if (sizeof(T) == 2) {
                    uint32_t W[8][4];
                    for (int r = 0; r < 8; r++)
                        for (int j = 0; j < 4; j++) W[r][j] = (uint32_t)v[r][2 * j] | ((uint32_t)v[r][2 * j + 1] << 16);
                    dbk::packed_filter_block16_h265<true>(W, sg, prm.max_v);
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
                    dbk::packed_filter_block_h265<true>(L, R, sg);
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
    if (cf == 1) run<T, 1>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else if (cf == 2) run<T, 2>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else if (cf == 3) run<T, 3>(plane, w, h, pitch_s, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride, ctb_log2, packed);
    else return 1;
    return 0;
}

extern "C" int g4_sim_filter_plane(void *plane, int w, int h, long pitch_bytes, int sample_bytes, int bit_depth, int chroma_format,
                                   const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride, int unit_log2,
                                   int c_qp_offset, int tc_offset_div2, const int8_t *offs, int offs_stride, int ctb_log2, int packed)
{
    const dbk::H265Prm prm = {tc_offset_div2 * 2, 0, c_qp_offset, bit_depth - 8, (1 << bit_depth) - 1};
    if (w < 8 || h < 8 || w % 4 || h % 4) return 2;
    qp = qp > 51 ? 51 : qp;
    if (sample_bytes == 1)
        return run_cf(chroma_format, (uint8_t *)plane, w, h, pitch_bytes, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride,
                      ctb_log2, packed);
    return run_cf(chroma_format, (uint16_t *)plane, w, h, pitch_bytes / 2, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, offs, offs_stride,
                  ctb_log2, packed);
}
