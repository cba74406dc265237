/*
 * rext_sim.cpp -- runs the KERNELS' per-block chroma arithmetic for 4:2:2 and 4:4:4 pictures (gpu_video_codec_amd/csrc:
 * deblock_h265.h, the 32-bit kernel's form; deblock_packed_h265.h / deblock_packed16.h, the packed kernels' one-QP form) on
 * the CPU over a whole plane, with the kernels' zero padding and bS guards.  TEST-ONLY: built by tests/test_rext_cpu.py,
 * never part of the product library.
 */
#include <cstdint>

#include "../../gpu_video_codec_amd/csrc/deblock_core.h"
#include "../../gpu_video_codec_amd/csrc/deblock_h265.h"
#define DBK_HOST_SIM 1
#include "../../gpu_video_codec_amd/csrc/deblock_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed_h265.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed16.h"

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

/* the blocks of a w x h chroma plane of format CF, in the kernels' order (any order gives the same result: blocks are
 * independent); packed = 1: the packed kernels' procedure -- one QP: the scalar tc of bS 2 as dbk_launch_packed_h265_cf derives it;
 * a QP map: the segment parameters of the format (h265_seg_params<true, CF>) */
template <typename T, int CF>
static void run(T *plane, int w, int h, long pitch_s, const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map,
                int map_stride, int unit_log2, const dbk::H265Prm &prm, int packed)
{
    constexpr int sx = dbk::ChromaFmt<CF>::sx, sy = dbk::ChromaFmt<CF>::sy;
    const int nbx = w / 8 + 1, nby = h / 8 + 1;
    const int tc_bs2 = dbk::h265_tc(dbk::clampi(dbk::h265_chroma_qp_cf<CF>(qp + prm.c_qp_offset) + 2 + prm.tc_off, 0, 53)) << prm.shift;
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            int v[8][8], entry[4], qpl[4];
            load_block(plane, pitch_s, w, h, bx, by, v);
            dbk::load_block_bs_h265(vbs4, hbs4, bx, by, nbx, nby, w / 8 + 1, w / 4, entry);
            if (packed) {
                dbk::H265Seg sg;
                if (map) { /* the QP-map kernels: the format's map positions, then h265_seg_params<true, CF> (QpC rule of the format) */
                    dbk::h265_block_qpl_xy(map, map_stride, unit_log2, sx, sy, w * sx, h * sy, bx * 8 - 4, by * 8 - 4, qp, qpl);
                    dbk::h265_seg_params<true, CF>(entry, qpl, prm, sg);
                } else {
                    for (int i = 0; i < 4; i++) {
                        sg.entry[i] = entry[i];
                        sg.beta[i] = 0;
                        sg.tc[i] = (entry[i] & dbk::kH265BsMask) == 2 ? tc_bs2 : 0;
                    }
                }
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
            } else {
                dbk::h265_block_qpl_xy(map, map_stride, unit_log2, sx, sy, w * sx, h * sy, bx * 8 - 4, by * 8 - 4, qp, qpl);
                dbk::filter_block_h265_chroma_cf<CF>(v, entry, qpl, prm);
            }
            store_block(plane, pitch_s, w, h, bx, by, v);
        }
}

extern "C" int rext_sim_filter_chroma(void *plane, int w, int h, long pitch_bytes, int sample_bytes, int bit_depth, int chroma_format,
                                      const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride,
                                      int unit_log2, int tc_offset_div2, int c_qp_offset, int packed)
{
    const dbk::H265Prm prm = {tc_offset_div2 * 2, 0, c_qp_offset, bit_depth - 8, (1 << bit_depth) - 1};
    qp = qp > 51 ? 51 : qp;
    if (chroma_format != 2 && chroma_format != 3) return 1;
    if (sample_bytes == 1) {
        if (chroma_format == 2) run<uint8_t, 2>((uint8_t *)plane, w, h, pitch_bytes, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, packed);
        else run<uint8_t, 3>((uint8_t *)plane, w, h, pitch_bytes, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, packed);
    } else {
        if (chroma_format == 2) run<uint16_t, 2>((uint16_t *)plane, w, h, pitch_bytes / 2, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, packed);
        else run<uint16_t, 3>((uint16_t *)plane, w, h, pitch_bytes / 2, vbs4, hbs4, qp, map, map_stride, unit_log2, prm, packed);
    }
    return 0;
}
