/*
 * sp_sim.cpp -- runs the semi-planar deblocking KERNELS' per-block procedure (gpu_video_codec_amd/csrc: deblock_sp.h's split and
 * merge of a row of sample pairs around the planar chroma block procedures, deblock_h265.h load_block_bs_h265_g4 with the kernels'
 * zero padding, deblock_sl.h for the offsets) on the CPU over a whole plane of interleaved Cb / Cr pairs.  TEST-ONLY: built by
 * tests/test_sp_cpu.py, never part of the product library.
 */
#include <cstdint>
#include <cstring>

#include "../../gpu_video_codec_amd/csrc/deblock_core.h"
#include "../../gpu_video_codec_amd/csrc/deblock_h265.h"
#define DBK_HOST_SIM 1
#include "../../gpu_video_codec_amd/csrc/deblock_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed_h265.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed16.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sp.h"

/* the kernels' loads: the block's row as the bytes of memory -- 16 (8-bit) or 32 (16-bit) bytes at pair 8 bx - 4 -- with zeros for a
 * half or a row outside the picture, where "outside" is what bx > 0, g4_right_in and the row test say of the block */
template <typename T>
static void load_rows(const T *plane, long pitch_s, int w, int h, int bx, int by, T (&raw)[8][16])
{
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, w);
    for (int r = 0; r < 8; r++)
        for (int i = 0; i < 16; i++) {
            const int y = by * 8 - 4 + r;
            const long s = 2L * (bx * 8 - 4) + i; /* sample of the row */
            raw[r][i] = ((i < 8 ? lv : rv) && y >= 0 && y < h) ? plane[(long)y * pitch_s + s] : 0;
        }
}
template <typename T>
static void store_rows(T *plane, long pitch_s, int w, int h, int bx, int by, const T (&raw)[8][16])
{
    const bool lv = bx > 0, rv = dbk::g4_right_in(bx, w);
    for (int r = 0; r < 8; r++)
        for (int i = 0; i < 16; i++) {
            const int y = by * 8 - 4 + r;
            const long s = 2L * (bx * 8 - 4) + i;
            if ((i < 8 ? lv : rv) && y >= 0 && y < h) plane[(long)y * pitch_s + s] = raw[r][i];
        }
}

/* form 0 = the 32-bit kernel (a component stride of 2), 1 = the packed kernels (deblock_sp.h).  offs == NULL: no per-slice offsets;
 * tc_off is ADDED to the pairs, as the kernels do */
template <typename T>
static void run(T *plane, int w, int h, long pitch_s, const uint8_t *vbs4, const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride,
                int unit_log2, int cb_off, int cr_off, int tc_off0, int shift, int max_v, const int8_t *offs, int offs_stride, int ctb_log2,
                int form)
{
    const int nbx = w / 8 + 1, nby = h / 8 + 1;
    auto pair = [&](int cx, int cy) {
        if (!offs) return 0u;
        const int8_t *p = offs + 2 * ((long)cy * offs_stride + cx);
        return (unsigned)(uint8_t)p[0] | ((unsigned)(uint8_t)p[1] << 8);
    };
    for (int by = 0; by < nby; by++)
        for (int bx = 0; bx < nbx; bx++) {
            T raw[8][16];
            int entry[4], qpl[4], cx[2], cy[2], tc_off[4], beta_off[4];
            load_rows(plane, pitch_s, w, h, bx, by, raw);
            dbk::load_block_bs_h265_g4(vbs4, hbs4, bx, by, w, h, w / 8 + 1, w / 4, entry);
            if (map) dbk::h265_block_qpl4(map, map_stride, unit_log2, 2, 2 * w, 2 * h, bx * 8 - 4, by * 8 - 4, qpl);
            else qpl[0] = qpl[1] = qpl[2] = qpl[3] = qp;
            dbk::h265_sl_ctbs<2, 2>(bx, by, 2 * w, 2 * h, ctb_log2, cx, cy);
            dbk::h265_sl_seg_offs(pair(cx[1], cy[0]), pair(cx[0], cy[1]), pair(cx[1], cy[1]), tc_off, beta_off);
            for (int s = 0; s < 4; s++) tc_off[s] += tc_off0;
            const dbk::H265Prm pb = {0, 0, cb_off, shift, max_v}, pr = {0, 0, cr_off, shift, max_v};
            if (form == 0) {
                for (int k = 0; k < 2; k++) {
                    int v[8][8];
                    for (int r = 0; r < 8; r++)
                        for (int c = 0; c < 8; c++) v[r][c] = raw[r][2 * c + k];
                    dbk::filter_block_h265_sl<1>(v, entry, qpl, k ? pr : pb, tc_off, beta_off);
                    for (int r = 0; r < 8; r++)
                        for (int c = 0; c < 8; c++) raw[r][2 * c + k] = (T)v[r][c];
                }
            } else {
                dbk::H265Seg sb, sr;
                dbk::h265_seg_params_sl<true, 1>(entry, qpl, pb, tc_off, beta_off, sb);
                dbk::h265_seg_params_sl<true, 1>(entry, qpl, pr, tc_off, beta_off, sr);
                if (sizeof(T) == 1) {
                    uint32_t D[8][4], Lb[8], Rb[8], Lr[8], Rr[8];
                    std::memcpy(D, raw, sizeof(D));
                    for (int r = 0; r < 8; r++) {
                        dbk::sp_split8<0>(D[r], Lb[r], Rb[r]);
                        dbk::sp_split8<1>(D[r], Lr[r], Rr[r]);
                    }
                    dbk::packed_filter_block_h265<true>(Lb, Rb, sb);
                    dbk::packed_filter_block_h265<true>(Lr, Rr, sr);
                    for (int r = 0; r < 8; r++) dbk::sp_merge8(Lb[r], Rb[r], Lr[r], Rr[r], D[r]);
                    std::memcpy(raw, D, sizeof(D));
                } else {
                    uint32_t D[8][8], Wb[8][4], Wr[8][4];
                    std::memcpy(D, raw, sizeof(D));
                    for (int r = 0; r < 8; r++) {
                        dbk::sp_split16<0>(D[r], Wb[r]);
                        dbk::sp_split16<1>(D[r], Wr[r]);
                    }
                    dbk::packed_filter_block16_h265<true>(Wb, sb, max_v);
                    dbk::packed_filter_block16_h265<true>(Wr, sr, max_v);
                    for (int r = 0; r < 8; r++) dbk::sp_merge16(Wb[r], Wr[r], D[r]);
                    std::memcpy(raw, D, sizeof(D));
                }
            }
            store_rows(plane, pitch_s, w, h, bx, by, raw);
        }
}

/* w x h = the samples per component; the plane holds 2 * w samples per row */
extern "C" int sp_sim_filter_plane(void *plane, int w, int h, long pitch_bytes, int sample_bytes, int bit_depth, const uint8_t *vbs4,
                                   const uint8_t *hbs4, int qp, const uint8_t *map, int map_stride, int unit_log2, int cb_qp_offset,
                                   int cr_qp_offset, int tc_offset_div2, const int8_t *offs, int offs_stride, int ctb_log2, int form)
{
    if (w < 8 || h < 8 || w % 4 || h % 4) return 2;
    if (form == 1 && bit_depth > 12) return 3; /* the packed kernels' range */
    qp = qp > 51 ? 51 : qp;
    const int shift = bit_depth - 8, max_v = (1 << bit_depth) - 1;
    if (sample_bytes == 1)
        run((uint8_t *)plane, w, h, pitch_bytes, vbs4, hbs4, qp, map, map_stride, unit_log2, cb_qp_offset, cr_qp_offset, tc_offset_div2 * 2,
            shift, max_v, offs, offs_stride, ctb_log2, form);
    else
        run((uint16_t *)plane, w, h, pitch_bytes / 2, vbs4, hbs4, qp, map, map_stride, unit_log2, cb_qp_offset, cr_qp_offset,
            tc_offset_div2 * 2, shift, max_v, offs, offs_stride, ctb_log2, form);
    return 0;
}

/* the split and the merge by themselves: a row of 16 (8-bit) / 16 (16-bit) samples -> the two components' 8 samples each and back */
extern "C" void sp_sim_split_merge(const void *row, int sample_bytes, void *comp0, void *comp1, void *back)
{
    if (sample_bytes == 1) {
        uint32_t d[4], o[4], l0, r0, l1, r1;
        std::memcpy(d, row, 16);
        dbk::sp_split8<0>(d, l0, r0);
        dbk::sp_split8<1>(d, l1, r1);
        const uint32_t c0[2] = {l0, r0}, c1[2] = {l1, r1};
        std::memcpy(comp0, c0, 8);
        std::memcpy(comp1, c1, 8);
        dbk::sp_merge8(l0, r0, l1, r1, o);
        std::memcpy(back, o, 16);
    } else {
        uint32_t d[8], o[8], w0[4], w1[4];
        std::memcpy(d, row, 32);
        dbk::sp_split16<0>(d, w0);
        dbk::sp_split16<1>(d, w1);
        std::memcpy(comp0, w0, 16);
        std::memcpy(comp1, w1, 16);
        dbk::sp_merge16(w0, w1, o);
        std::memcpy(back, o, 32);
    }
}
