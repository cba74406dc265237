/*
 * sao_scale_sim.cpp -- csrc/sao_pick_os.h compiled for the CPU: a stand-alone program that runs SAO estimation with
 * log2_sao_offset_scale over one CTB grid as the kernels of sao_pick_os.hip do.  Per CTB a "wave" of 64 lanes: every step of the
 * procedure is executed for ALL 64 lanes before the next begins, and between the steps the lanes exchange keys the way the kernel's
 * cross-lane moves do -- lane l takes the key of lane l ^ m, m = 1, 2, 4, ...  Then, for the decision, sao_decide.h's merge_ctb
 * anti-diagonal by anti-diagonal in chunks of 256, as tests/sao_decide_sim.  tests/test_sao_scale_cpu.py writes the operands into a
 * file, runs the program -- plain and under -fsanitize=address,undefined -- and compares what comes back with tests/sao_scale_ref.py.
 * Every operand lives in a heap block of exactly its size: a read or write outside it is the sanitizer's to find.
 *
 *   sao_scale_sim IN OUT   IN: int32 ctbs_x, ctbs_y, chroma, bit_depth_luma, bit_depth_chroma, lambda_q8_luma, lambda_q8_chroma,
 *                          has_slice_idx, has_tile_idx, log2_scale_luma, log2_scale_chroma, mode; n x 96 int32 (first array) and, if
 *                          chroma, the second and (mode 0) the third; n uint16 (slice_idx) and n uint16 (tile_idx) where present.
 *                          n = ctbs_x * ctbs_y, every array tight.
 *                          mode 0, the decision: Y, Cb, Cr.  OUT: n x 6 bytes (Y) and, if chroma, Cb's and Cr's; n x 32 bytes of records
 *                          mode 1, the pick: a and, if chroma, b beside it, with the luma depth, lambda and scale.  OUT: n x 6 bytes (a)
 *                          and, if chroma, b's; n int64 delta_d
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sao_pick_os.h"

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

/* the exchange: after it every lane of a group of `width` neighbouring lanes holds the group's least key */
void group_min(saoos::Key (&k)[kLanes], int width)
{
    for (int m = 1; m < width; m <<= 1) {
        saoos::Key next[kLanes];
        for (int lane = 0; lane < kLanes; lane++) next[lane] = saoos::key_min(k[lane], k[lane ^ m]);
        std::memcpy(k, next, sizeof(next));
    }
}

/* one component: every lane's choice; the wave agrees on it */
saoos::Choice single(const saoos::BinPick *p, long long lambda)
{
    saoos::Key k[kLanes];
    for (int lane = 0; lane < kLanes; lane++) k[lane] = saoos::single_key(p, lane, lambda);
    group_min(k, 64);
    saoos::Choice c[kLanes];
    for (int lane = 0; lane < kLanes; lane++) c[lane] = saoos::single_choice(k[lane]);
    for (int lane = 1; lane < kLanes; lane++)
        if (c[lane].type != c[0].type || c[lane].cls_a != c[0].cls_a || c[lane].cls_b != c[0].cls_b || c[lane].cost != c[0].cost) std::abort();
    return c[0];
}

/* Cr beside Cb: lane 0's choice -- it sits in the first group of both reductions and takes Cr's least key from lane 32 */
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
    static_assert(sizeof(DbkSaoCtb) == 6 && sizeof(DbkSaoDecision) == 32, "the entries of the C ABI");
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    std::vector<uint8_t> buf;
    int32_t hd[12];
    if (!read_all(argv[1], buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int X = hd[0], Y = hd[1], mode = hd[11];
    const bool chroma = hd[2] != 0;
    const int comps = chroma ? (mode == 0 ? 3 : 2) : 1;
    const size_t n = (size_t)X * Y, one = n * saostats::kBins;
    if (X <= 0 || Y <= 0 || (mode != 0 && mode != 1) || buf.size() != sizeof(hd) + one * 4 * comps + n * 2 * ((hd[7] ? 1 : 0) + (hd[8] ? 1 : 0))) return 3;
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
    std::vector<DbkSaoCtb> prm[3];
    for (int c = 0; c < comps; c++) prm[c].resize(n);
    std::vector<DbkSaoDecision> dec(mode == 0 ? n : 0);
    std::vector<long long> dd(mode == 1 ? n : 0);
    if (!dec.empty()) std::memset(dec.data(), 0xA5, n * sizeof(DbkSaoDecision)); /* the procedure writes every byte of every record */

    DbkSaoDecideOsArgs o = {};
    DbkSaoDecideArgs &a = o.d;
    a.stats_y = st[0].data();
    a.stats_cb = comps == 3 ? st[1].data() : nullptr;
    a.stats_cr = comps == 3 ? st[2].data() : nullptr;
    a.stats_stride = a.params_stride = a.decision_stride = a.idx_stride = X;
    a.ctbs_x = X; a.ctbs_y = Y; a.n_frames = 1;
    a.max_offset_luma = max_offset(hd[3]); a.max_offset_chroma = max_offset(hd[4]);
    a.lambda_luma = hd[5]; a.lambda_chroma = hd[6];
    a.slice_idx = hd[7] ? idx[0].data() : nullptr;
    a.tile_idx = hd[8] ? idx[1].data() : nullptr;
    a.params_y = prm[0].data();
    a.params_cb = comps == 3 ? prm[1].data() : nullptr;
    a.params_cr = comps == 3 ? prm[2].data() : nullptr;
    a.decision = dec.data();
    o.log2_scale_luma = hd[9]; o.log2_scale_chroma = hd[10];

    DbkSaoPickOsArgs po = {};
    DbkSaoPickArgs &pa = po.p;
    pa.stats_a = st[0].data();
    pa.stats_b = comps == 2 ? st[1].data() : nullptr;
    pa.stats_stride = pa.params_stride = X;
    pa.ctbs_x = X; pa.ctbs_y = Y; pa.n_frames = 1;
    pa.max_offset = max_offset(hd[3]); pa.lambda = hd[5];
    pa.params_a = prm[0].data();
    pa.params_b = comps == 2 ? prm[1].data() : nullptr;
    pa.delta_d = dd.data();
    po.log2_scale = hd[9];

    for (int cy = 0; cy < Y; cy++)
        for (int cx = 0; cx < X; cx++) {
            saoos::BinPick pk[3][saostats::kPickBins];
            const size_t at = ((size_t)cy * X + cx) * saostats::kBins;
            for (int lane = 0; lane < saostats::kPickBins; lane++)
                for (int c = 0; c < comps; c++) {
                    const bool luma = mode == 1 || c == 0;
                    pk[c][lane] = saoos::pick_bin(st[c].data() + at, lane, luma ? a.max_offset_luma : a.max_offset_chroma,
                                                  luma ? o.log2_scale_luma : o.log2_scale_chroma, luma ? a.lambda_luma : a.lambda_chroma);
                }
            if (mode == 1) {
                const saoos::Choice c = comps == 2 ? joint(pk[0], pk[1], pa.lambda) : single(pk[0], pa.lambda);
                saoos::write_pick(pa, 0, cx, cy, pk[0], comps == 2 ? pk[1] : nullptr, c);
            } else {
                const saoos::Choice y = single(pk[0], a.lambda_luma);
                saoos::Choice c = {};
                if (comps == 3) c = joint(pk[1], pk[2], a.lambda_chroma);
                saoos::write_new(a, 0, cx, cy, pk[0], pk[1], pk[2], y, c);
            }
        }
    if (mode == 0)
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
    for (int c = 0; c < comps; c++) ok = std::fwrite(prm[c].data(), sizeof(DbkSaoCtb), n, f) == n && ok;
    if (mode == 0) ok = std::fwrite(dec.data(), sizeof(DbkSaoDecision), n, f) == n && ok;
    else ok = std::fwrite(dd.data(), sizeof(long long), n, f) == n && ok;
    return std::fclose(f) == 0 && ok ? 0 : 4;
}
