/*
 * sao_slice_sim.cpp -- csrc/sao_slice.h compiled for the CPU: a stand-alone program that runs the SAO decision under slice-level
 * flags, and the choice of those flags, over one CTB grid as the kernels of sao_slice.hip do.  Per CTB a "wave" of 64 lanes runs the
 * NEW step -- every step for ALL 64 lanes before the next, the keys exchanged as the kernel's cross-lane moves do (lane l takes the
 * key of lane l ^ m), as tests/sao_scale_sim.  Then the walk, anti-diagonal by anti-diagonal in chunks of 256: under given flags
 * sao_decide.h's merge_ctb; for the choice the (pair, CTB) items of a diagonal, each adding the four 32-bit limbs of its J to 64-bit
 * sums per slice, then the carry step and the choice per slice, then the final copy per CTB.  tests/test_sao_slice_flags_cpu.py
 * writes the operands into a file, runs the program -- plain and under -fsanitize=address,undefined -- and compares what comes back
 * with tests/sao_slice_ref.py.  Every operand, the workspace included, lives in a heap block of exactly its size.
 *
 *   sao_slice_sim IN OUT   IN: int32 ctbs_x, ctbs_y, chroma, bit_depth_luma, bit_depth_chroma, lambda_q8_luma, lambda_q8_chroma,
 *                          has_slice_idx, has_tile_idx, log2_scale_luma, log2_scale_chroma, mode, n_slices; n x 96 int32 (Y) and, if
 *                          chroma, Cb's and Cr's; n uint16 (slice_idx) and n uint16 (tile_idx) where present; mode 0: n_slices flag
 *                          bytes.  n = ctbs_x * ctbs_y, every array tight.
 *                          OUT: n x 6 bytes (Y) and, if chroma, Cb's and Cr's; n x 32 bytes of records; mode 1 (the choice): n_slices
 *                          flag bytes and n_slices x 72 bytes of slice records
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sao_slice.h"

namespace {

constexpr int kLanes = 64;

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

void group_min(saoos::Key (&k)[kLanes], int width)
{
    for (int m = 1; m < width; m <<= 1) {
        saoos::Key next[kLanes];
        for (int lane = 0; lane < kLanes; lane++) next[lane] = saoos::key_min(k[lane], k[lane ^ m]);
        std::memcpy(k, next, sizeof(next));
    }
}

saoos::Choice single(const saoos::BinPick *p, long long lambda)
{
    saoos::Key k[kLanes];
    for (int lane = 0; lane < kLanes; lane++) k[lane] = saoos::single_key(p, lane, lambda);
    group_min(k, 64);
    return saoos::single_choice(k[0]);
}

saoos::Choice joint(const saoos::BinPick *a, const saoos::BinPick *b, long long lambda)
{
    saoos::Key e[kLanes], k[kLanes];
    for (int lane = 0; lane < kLanes; lane++) e[lane] = saoos::joint_edge_key(a, b, lane, lambda);
    group_min(e, 8);
    for (int lane = 0; lane < kLanes; lane++) k[lane] = saoos::joint_band_key(a, b, lane);
    group_min(k, 32);
    return saoos::joint_choice(e[0], k[0], k[32], lambda);
}

} /* namespace */

int main(int argc, char **argv)
{
    static_assert(sizeof(DbkSaoCtb) == 6 && sizeof(DbkSaoDecision) == 32 && sizeof(DbkSaoSliceRecord) == 72, "the entries of the C ABI");
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    std::vector<uint8_t> buf;
    int32_t hd[13];
    if (!read_all(argv[1], buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int X = hd[0], Y = hd[1], mode = hd[11], S = hd[12];
    const bool chroma = hd[2] != 0;
    const int comps = chroma ? 3 : 1;
    const size_t n = (size_t)X * Y, one = n * saostats::kBins;
    if (X <= 0 || Y <= 0 || S <= 0 || (mode != 0 && mode != 1) || (mode == 1 && S > saoslice::kMaxSlices)) return 3;
    if (buf.size() != sizeof(hd) + one * 4 * comps + n * 2 * ((hd[7] ? 1 : 0) + (hd[8] ? 1 : 0)) + (mode == 0 ? (size_t)S : 0)) return 3;
    const uint8_t *p = buf.data() + sizeof(hd);
    std::vector<int32_t> st[3];
    for (int c = 0; c < comps; c++, p += one * 4) {
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
    std::vector<uint8_t> flags((size_t)S, 0xA5);
    if (mode == 0) std::memcpy(flags.data(), p, (size_t)S);
    std::vector<DbkSaoCtb> prm[3];
    for (int c = 0; c < comps; c++) {
        prm[c].resize(n);
        std::memset(prm[c].data(), 0xA5, n * sizeof(DbkSaoCtb));
    }
    std::vector<DbkSaoDecision> dec(n);
    std::memset(dec.data(), 0xA5, n * sizeof(DbkSaoDecision)); /* the procedure writes every byte of every output */
    std::vector<DbkSaoSliceRecord> rec((size_t)(mode == 1 ? S : 0));
    if (!rec.empty()) std::memset(rec.data(), 0xA5, rec.size() * sizeof(DbkSaoSliceRecord));
    std::vector<uint8_t> ws(mode == 1 ? n * saoslice::kStateBytes : 0, 0xA5); /* exactly what the size function says, before rounding */

    DbkSaoSliceArgs s = {};
    DbkSaoDecideArgs &a = s.o.d;
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
    s.o.log2_scale_luma = hd[9]; s.o.log2_scale_chroma = hd[10];
    s.n_slices = S;
    if (mode == 0) s.flags_in = flags.data();
    else {
        s.flags_out = flags.data();
        s.record = rec.data();
        s.ws_decision = reinterpret_cast<DbkSaoDecision *>(ws.data());
        s.ws_params = reinterpret_cast<DbkSaoCtb *>(s.ws_decision + 3 * n);
    }

    /* NEW: one wave per CTB */
    for (int cy = 0; cy < Y; cy++)
        for (int cx = 0; cx < X; cx++) {
            saoos::BinPick pk[3][saostats::kPickBins];
            const size_t at = ((size_t)cy * X + cx) * saostats::kBins;
            for (int lane = 0; lane < saostats::kPickBins; lane++)
                for (int c = 0; c < comps; c++)
                    pk[c][lane] = saoos::pick_bin(st[c].data() + at, lane, c == 0 ? a.max_offset_luma : a.max_offset_chroma,
                                                  c == 0 ? s.o.log2_scale_luma : s.o.log2_scale_chroma, c == 0 ? a.lambda_luma : a.lambda_chroma);
            const saoos::Choice y = single(pk[0], a.lambda_luma);
            saoos::Choice c = {};
            if (chroma) c = joint(pk[1], pk[2], a.lambda_chroma);
            if (mode == 0) saoslice::new_masked(a, 0, cx, cy, pk[0], pk[1], pk[2], y, c, saoslice::pair_given(s, 0, cx, cy));
            else saoslice::new_states(s, 0, cx, cy, pk[0], pk[1], pk[2], y, c);
        }

    if (mode == 0) {
        for (int d = 1; d <= X + Y - 2; d++) {
            int cy0;
            const int cnt = saodecide::diagonal(X, Y, d, cy0);
            for (int chunk = 0; chunk < cnt; chunk += saodecide::kChunk)
                for (int t = 0; t < saodecide::kChunk; t++) /* the threads of the workgroup */
                    if (chunk + t < cnt) saodecide::merge_ctb(a, 0, d - (cy0 + chunk + t), cy0 + chunk + t);
        }
    } else {
        std::vector<unsigned long long> sums((size_t)S * saoslice::kSums, 0); /* the LDS of the walk's workgroup */
        std::vector<unsigned> count((size_t)S, 0);
        const int n_pairs = saoslice::pairs(s);
        for (int d = 0; d <= X + Y - 2; d++) {
            int cy0;
            const int cnt = saodecide::diagonal(X, Y, d, cy0);
            for (int chunk = 0; chunk < cnt * n_pairs; chunk += saodecide::kChunk)
                for (int t = 0; t < saodecide::kChunk; t++) {
                    const int i = chunk + t;
                    if (i >= cnt * n_pairs) continue;
                    const int pair = i / cnt + 1, k = i - (pair - 1) * cnt, cx = d - (cy0 + k), cy = cy0 + k;
                    const unsigned sl = saoslice::slice_of(a, 0, cx, cy);
                    if (sl >= (unsigned)S) continue;
                    const saodecide::wide j = saoslice::walk_ctb(saoslice::pair_state(s, pair), 0, cx, cy);
                    for (int l = 0; l < 4; l++) sums[(size_t)saoslice::sum_at(sl, pair, l)] += saoslice::limb(j, l);
                    if (pair == 1) count[sl]++;
                }
        }
        for (int sl = 0; sl < S; sl++) {
            DbkSaoSliceRecord r;
            flags[(size_t)sl] = (uint8_t)saoslice::choose(sums.data() + (size_t)sl * saoslice::kSums, count[(size_t)sl], chroma, r);
            rec[(size_t)sl] = r;
        }
        for (size_t i = 0; i < n; i++) saoslice::final_ctb(s, 0, (int)(i % X), (int)(i / X));
    }

    FILE *f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    bool ok = true;
    for (int c = 0; c < comps; c++) ok = std::fwrite(prm[c].data(), sizeof(DbkSaoCtb), n, f) == n && ok;
    ok = std::fwrite(dec.data(), sizeof(DbkSaoDecision), n, f) == n && ok;
    if (mode == 1) {
        ok = std::fwrite(flags.data(), 1, (size_t)S, f) == (size_t)S && ok;
        ok = std::fwrite(rec.data(), sizeof(DbkSaoSliceRecord), (size_t)S, f) == (size_t)S && ok;
    }
    return std::fclose(f) == 0 && ok ? 0 : 4;
}
