/*
 * fused_sp_sim.cpp -- runs the per-lane procedures of the fused deblocking + SAO kernels for a semi-planar chroma plane
 * (gpu_video_codec_amd/csrc/deblock_sao_sp_fused.h) on the CPU, tile by tile as the kernel does: stage 1 of every lane of a tile
 * into a host array that stands for the LDS tile -- rims included, the array filled with a poison byte first -- then, "after the
 * barrier", stage 2 out of that array into the destination, unit by unit with the wave's two ballots.  The loads are the kernel's:
 * a half or a row of a block outside the picture is zeros, whatever memory holds there; the operand fetch is deblock_sp_dev.h's
 * done with the host forms of the same procedures (deblock_h265.h, deblock_sl.h), as tests/sp_sim does it.
 *
 * A stand-alone program (the Makefile's asan target builds it with -fsanitize=address,undefined):
 *     fused_sp_sim JOB OUT
 * JOB: 24 int64 -- w h pitch sample_bytes bit_depth qp use_map map_stride unit_log2 cb_qp_offset cr_qp_offset tc_off beta_off
 *      use_pairs offs_stride sl_ctb_log2 params_stride ctb_log2 keep_stride nox_stride pad_rows lds_poison 0 0 -- then nine blobs, each
 *      an int64 byte count (0 = absent) and the bytes: the padded source (pad_rows + h + pad_rows rows of pitch bytes), vertical bS,
 *      horizontal bS, QP map, per-slice pairs, Cb parameters, Cr parameters, keep map, boundary bytes.
 * OUT: the destination, the size of the padded source, every byte 0x5A that the kernel would not write.
 * TEST-ONLY: built by tests/test_fused_sp_cpu.py, never part of the product library.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gpu_video_codec_amd/csrc/deblock_core.h"
#include "../../gpu_video_codec_amd/csrc/deblock_h265.h"
#define DBK_HOST_SIM 1
#include "../../gpu_video_codec_amd/csrc/deblock_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed_h265.h"
#include "../../gpu_video_codec_amd/csrc/deblock_packed16.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sl_packed.h"
#include "../../gpu_video_codec_amd/csrc/deblock_sao_sp_fused.h"

namespace {

struct Job {
    int64_t w, h, pitch, sb, depth, qp, use_map, map_stride, unit_log2, cb_off, cr_off, tc_off, beta_off, use_pairs, offs_stride, sl_ctb_log2,
        pstride, ctb_log2, keep_stride, nox_stride, pad_rows, lds_poison, r0, r1;
};
typedef std::vector<uint8_t> Blob;

/* the buffer resource of the kernel: bytes [0, pitch * h) of the plane, zero beyond */
struct Plane {
    const uint8_t *p;
    int64_t bytes;
    uint32_t rd32(int64_t off) const
    {
        uint32_t v = 0u;
        if (off >= 0 && off + 4 <= bytes) std::memcpy(&v, p + off, 4);
        return v;
    }
};

template <int SB>
void run(const Job &j, const Blob &src, const Blob &vbs, const Blob &hbs, const Blob &map, const Blob &offs, const Blob &pcb, const Blob &pcr,
         const Blob &keep, const Blob &nox, Blob &dst)
{
    typedef spf::Geo<SB> G;
    const int w = (int)j.w, h = (int)j.h, nbx = w / 8 + 1, nby = h / 8 + 1, shift = (int)j.depth - 8, max_v = (1 << j.depth) - 1;
    const int64_t pitch = j.pitch, org = j.pad_rows * pitch;
    const Plane pl = {src.data() + org, pitch * h};
    uint8_t *const out = dst.data() + org;
    const DbkSaoCtb *cb_prm = reinterpret_cast<const DbkSaoCtb *>(pcb.data()), *cr_prm = reinterpret_cast<const DbkSaoCtb *>(pcr.data());
    const spf::Pic pic = {w, h, (int)j.ctb_log2, max_v, (int)j.depth - 5};
    auto pair = [&](int cx, int cy) {
        if (!j.use_pairs) return 0u;
        const int8_t *p = reinterpret_cast<const int8_t *>(offs.data()) + 2 * ((long)cy * j.offs_stride + cx);
        return (unsigned)(uint8_t)p[0] | ((unsigned)(uint8_t)p[1] << 8);
    };
    alignas(16) static uint8_t tile[G::kLds];
    for (int Y0 = 0; Y0 < h; Y0 += G::kTileH)
        for (int X0 = 0; X0 < w; X0 += G::kTileW) {
            std::memset(tile, (int)j.lds_poison, sizeof(tile));
            /* ---- stage 1: every lane of the tile ---- */
            for (int t = 0; t < G::kLanes; t++) {
                const int lby = t / G::kBlocksX, lbx = t - G::kBlocksX * lby;
                const int bx = (X0 >> 3) + lbx, by = (Y0 >> 3) + lby;
                const bool active = bx < nbx && by < nby;
                const bool lv = active && bx > 0, rv = active && dbk::g4_right_in(bx, w);
                const int y0 = by * 8 - 4;
                uint32_t D[8][4 * SB];
                for (int r = 0; r < 8; r++) {
                    const bool yv = (unsigned)(y0 + r) < (unsigned)h;
                    const int64_t off = (int64_t)(y0 + r) * pitch + (int64_t)bx * 16 * SB - 8 * SB;
                    for (int i = 0; i < 4 * SB; i++) D[r][i] = (yv && (i < 2 * SB ? lv : rv)) ? pl.rd32(off + 4 * i) : 0u;
                }
                const int obx = active ? bx : 0, oby = active ? by : 0; /* an idle lane takes the operands of block (0, 0) */
                int entry[4], qpl[4], cx[2], cy[2], tc_off[4], beta_off[4];
                dbk::load_block_bs_h265_g4(vbs.data(), hbs.data(), obx, oby, w, h, w / 8 + 1, w / 4, entry);
                if (j.use_map) dbk::h265_block_qpl4(map.data(), (int)j.map_stride, (int)j.unit_log2, 2, 2 * w, 2 * h, obx * 8 - 4, oby * 8 - 4, qpl);
                else qpl[0] = qpl[1] = qpl[2] = qpl[3] = (int)(j.qp > 51 ? 51 : j.qp);
                dbk::h265_sl_ctbs<2, 2>(obx, oby, 2 * w, 2 * h, (int)j.sl_ctb_log2, cx, cy);
                dbk::h265_sl_seg_offs(pair(cx[1], cy[0]), pair(cx[0], cy[1]), pair(cx[1], cy[1]), tc_off, beta_off);
                for (int s = 0; s < 4; s++) {
                    tc_off[s] += (int)j.tc_off;
                    beta_off[s] += (int)j.beta_off;
                }
                const dbk::H265Prm pb = {0, 0, (int)j.cb_off, SB == 1 ? 0 : shift, SB == 1 ? 255 : max_v},
                                   pr = {0, 0, (int)j.cr_off, SB == 1 ? 0 : shift, SB == 1 ? 255 : max_v};
                dbk::H265Seg sb, sr;
                dbk::h265_seg_params_sl<true, 1>(entry, qpl, pb, tc_off, beta_off, sb);
                dbk::h265_seg_params_sl<true, 1>(entry, qpl, pr, tc_off, beta_off, sr);
                spf::deblock_to_tile(D, sb, sr, max_v, tile, lbx, lby);
            }
            /* ---- the barrier; stage 2: the tile's units, each by one wave ---- */
            for (int u = 0; u < G::kUnits; u++) {
                struct Lane {
                    int qx, qy, x, ys;
                    uint32_t m;
                    bool on, w4;
                } L[64];
                bool masked = false;
                for (int l = 0; l < 64; l++) {
                    Lane &a = L[l];
                    spf::unit_block<SB>(u, l, a.qx, a.qy);
                    a.x = X0 + a.qx;
                    a.ys = Y0 + a.qy;
                    a.on = a.x < w && a.ys < h;
                    if (!a.on) continue;
                    const uint32_t b = j.nox_stride ? nox[(size_t)(a.ys >> j.ctb_log2) * j.nox_stride + (a.x >> j.ctb_log2)] : 0u;
                    a.w4 = a.x + 8 > w;
                    a.m = saonox::block_mask<2>(b, a.x, a.ys, w, h, (int)j.ctb_log2) | (a.w4 ? saonox::W4 : 0u);
                    masked |= a.m != 0u;
                }
                for (int l = 0; l < 64; l++) {
                    const Lane &a = L[l];
                    if (!a.on) continue;
                    const size_t at = (size_t)(a.ys >> j.ctb_log2) * j.pstride + (a.x >> j.ctb_log2);
                    const bool kept = j.keep_stride && keep[(size_t)(a.ys >> 3) * j.keep_stride + (a.x >> 3)];
                    if constexpr (SB == 1) {
                        auto store = [&](int r, const uint32_t (&d)[4]) {
                            std::memcpy(out + (int64_t)(a.ys + r) * pitch + (int64_t)a.x * 2, d, a.w4 ? 8 : 16);
                        };
                        spf::sao_from_tile8(tile, a.qx, a.qy, a.x, a.ys, pic, cb_prm[at], cr_prm[at], kept, a.m, masked, store);
                    } else {
                        auto store = [&](int r, const uint32_t (&d)[8]) {
                            std::memcpy(out + (int64_t)(a.ys + r) * pitch + (int64_t)a.x * 4, d, a.w4 ? 16 : 32);
                        };
                        spf::sao_from_tile16(tile, a.qx, a.qy, a.x, a.ys, pic, cb_prm[at], cr_prm[at], kept, a.m, masked, store);
                    }
                }
            }
        }
}

bool read_blob(FILE *f, Blob &b)
{
    int64_t n;
    if (std::fread(&n, 8, 1, f) != 1 || n < 0) return false;
    b.resize((size_t)n);
    return n == 0 || std::fread(b.data(), 1, (size_t)n, f) == (size_t)n;
}

} /* namespace */

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Job j;
    Blob src, vbs, hbs, map, offs, pcb, pcr, keep, nox;
    bool ok = std::fread(&j, sizeof(j), 1, f) == 1;
    for (Blob *b : {&src, &vbs, &hbs, &map, &offs, &pcb, &pcr, &keep, &nox}) ok = ok && read_blob(f, *b);
    std::fclose(f);
    if (!ok) return 2;
    if (j.w < 8 || j.h < 8 || j.w % 4 || j.h % 4 || j.depth > 12 || (j.sb != 1 && j.sb != 2) || (j.sb == 1) != (j.depth == 8)) return 3;
    if ((int64_t)src.size() != (2 * j.pad_rows + j.h) * j.pitch || j.pitch < 2 * j.w * j.sb) return 3;
    if (!j.use_map) map.clear();
    if (!j.keep_stride) keep.clear();
    if (!j.nox_stride) nox.clear();
    Blob dst(src.size(), 0x5A);
    if (j.sb == 1) run<1>(j, src, vbs, hbs, map, offs, pcb, pcr, keep, nox, dst);
    else run<2>(j, src, vbs, hbs, map, offs, pcb, pcr, keep, nox, dst);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(dst.data(), 1, dst.size(), f) != dst.size()) return 2;
    std::fclose(f);
    return 0;
}
