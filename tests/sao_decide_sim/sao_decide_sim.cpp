/*
 * sao_decide_sim.cpp -- csrc/sao_decide.h compiled for the CPU: a stand-alone program that runs the SAO decision over one CTB grid as
 * the kernels of sao_decide.hip do -- new_ctb for every CTB (with the 48 bin picks per component a wave's lanes make), then merge_ctb
 * anti-diagonal by anti-diagonal, each diagonal in chunks of 256 CTBs.  tests/test_sao_decide_cpu.py writes the operands into a file,
 * runs the program -- plain and under -fsanitize=address,undefined -- and compares what comes back with tests/sao_decide_ref.py.
 * Every operand lives in a heap block of exactly its size: a read or write outside it is the sanitizer's to find.
 *
 *   sao_decide_sim IN OUT   IN: int32 ctbs_x, ctbs_y, chroma, bit_depth_luma, bit_depth_chroma, lambda_q8_luma, lambda_q8_chroma,
 *                           has_slice_idx, has_tile_idx; n x 96 int32 (Y) and, if chroma, again (Cb) and again (Cr); n uint16
 *                           (slice_idx) and n uint16 (tile_idx) where present.  n = ctbs_x * ctbs_y, every array tight.
 *                           OUT: n x 6 bytes (Y) and, if chroma, Cb's and Cr's; n x 32 bytes of records
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sao_decide.h"

namespace {

bool read_all(const char *path, std::vector<uint8_t> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize((size_t)n);
    const bool ok = n == 0 || std::fread(out.data(), 1, (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok;
}

int max_offset(int bd) { return (1 << ((bd < 10 ? bd : 10) - 5)) - 1; }

} /* namespace */

int main(int argc, char **argv)
{
    static_assert(sizeof(DbkSaoCtb) == 6 && sizeof(DbkSaoDecision) == 32, "the entries of the C ABI");
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    std::vector<uint8_t> buf;
    int32_t hd[9];
    if (!read_all(argv[1], buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int X = hd[0], Y = hd[1];
    const bool chroma = hd[2] != 0;
    const size_t n = (size_t)X * Y, one = n * saostats::kBins;
    if (X <= 0 || Y <= 0 || buf.size() != sizeof(hd) + one * 4 * (chroma ? 3 : 1) + n * 2 * ((hd[7] ? 1 : 0) + (hd[8] ? 1 : 0))) return 3;
    const uint8_t *p = buf.data() + sizeof(hd);
    std::vector<int32_t> st[3];
    for (int c = 0; c < (chroma ? 3 : 1); c++, p += one * 4) {
        st[c].resize(one);
        std::memcpy(st[c].data(), p, one * 4);
    }
    std::vector<uint16_t> idx[2];
    for (int k = 0; k < 2; k++)
        if (hd[7 + k]) {
            idx[k].resize(n);
            std::memcpy(idx[k].data(), p, n * 2);
            p += n * 2;
        }
    std::vector<DbkSaoCtb> prm[3];
    for (int c = 0; c < (chroma ? 3 : 1); c++) prm[c].resize(n);
    std::vector<DbkSaoDecision> dec(n);
    std::memset(dec.data(), 0xA5, n * sizeof(DbkSaoDecision)); /* the procedure writes every byte of every record */

    DbkSaoDecideArgs a = {};
    a.stats_y = st[0].data();
    a.stats_cb = chroma ? st[1].data() : nullptr;
    a.stats_cr = chroma ? st[2].data() : nullptr;
    a.stats_stride = a.params_stride = a.decision_stride = a.idx_stride = X;
    a.ctbs_x = X; a.ctbs_y = Y; a.n_frames = 1;
    a.max_offset_luma = max_offset(hd[3]); a.max_offset_chroma = max_offset(hd[4]);
    a.lambda_luma = hd[5]; a.lambda_chroma = hd[6];
    a.slice_idx = hd[7] ? idx[0].data() : nullptr;
    a.tile_idx = hd[8] ? idx[1].data() : nullptr;
    a.params_y = prm[0].data();
    a.params_cb = chroma ? prm[1].data() : nullptr;
    a.params_cr = chroma ? prm[2].data() : nullptr;
    a.decision = dec.data();

    for (int cy = 0; cy < Y; cy++)
        for (int cx = 0; cx < X; cx++) {
            saostats::BinPick pk[3][saostats::kPickBins];
            const size_t at = ((size_t)cy * X + cx) * saostats::kBins;
            for (int lane = 0; lane < saostats::kPickBins; lane++) {
                pk[0][lane] = saostats::pick_bin(a.stats_y + at, lane, a.max_offset_luma, a.lambda_luma);
                if (chroma) {
                    pk[1][lane] = saostats::pick_bin(a.stats_cb + at, lane, a.max_offset_chroma, a.lambda_chroma);
                    pk[2][lane] = saostats::pick_bin(a.stats_cr + at, lane, a.max_offset_chroma, a.lambda_chroma);
                }
            }
            saodecide::new_ctb(a, 0, cx, cy, pk[0], pk[1], pk[2]);
        }
    for (int d = 1; d <= X + Y - 2; d++) {
        int cy0;
        const int cnt = saodecide::diagonal(X, Y, d, cy0);
        for (int chunk = 0; chunk < cnt; chunk += saodecide::kChunk)
            for (int t = 0; t < saodecide::kChunk; t++) /* the threads of the workgroup */
                if (chunk + t < cnt) saodecide::merge_ctb(a, 0, d - (cy0 + chunk + t), cy0 + chunk + t);
    }

    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    bool ok = true;
    for (int c = 0; c < (chroma ? 3 : 1); c++) ok = std::fwrite(prm[c].data(), sizeof(DbkSaoCtb), n, f) == n && ok;
    ok = std::fwrite(dec.data(), sizeof(DbkSaoDecision), n, f) == n && ok;
    return std::fclose(f) == 0 && ok ? 0 : 4;
}
