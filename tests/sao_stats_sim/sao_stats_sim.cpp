/*
 * sao_stats_sim.cpp -- csrc/sao_stats.h compiled for the CPU: a stand-alone program that runs the per-block procedure of the SAO
 * statistics kernel over a whole plane, block by block as the kernel's lanes do, and the pick procedure over a list of CTBs.
 * tests/test_sao_stats_cpu.py writes the operands into a file, runs the program -- plain and under -fsanitize=address,undefined --
 * and compares what comes back with tests/sao_stats_ref.py.  Planes live in heap blocks of exactly their size: a read outside
 * them is the sanitizer's to find.
 *
 *   sao_stats_sim stats IN OUT   IN: int32 w, h, sample_bytes, bit_depth, lw, lh, has_keep, has_nox, pitch (samples); rec, org (h rows of
 *                                `pitch` samples), keep (ceil(h/8) x ceil(w/8)), nox (CTB rows x columns).  OUT: 96 int32 per CTB
 *   sao_stats_sim pick IN OUT    IN: int32 bit_depth, lambda_q8, n, joint; n x 96 int32 (a), and again (b) if joint.
 *                                OUT: n x 6 bytes (a), n x 6 bytes (b, if joint), n x int64 delta_d
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sao_stats.h"

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

bool write_all(const char *path, const void *p, size_t n)
{
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, n, f) == n;
    return std::fclose(f) == 0 && ok;
}

template <typename T>
void stats_plane(const T *rec, const T *org, int pitch, const saostats::Geo &g, const uint8_t *keep, const uint8_t *nox, int32_t *out)
{
    const int cols = (g.w + (1 << g.lw) - 1) >> g.lw, rows = (g.h + (1 << g.lh) - 1) >> g.lh, kw = (g.w + 7) / 8;
    std::vector<int32_t> work((size_t)rows * cols * 2 * saostats::kSlots, 0); /* the working histograms, as the kernel keeps them in LDS */
    for (int y0 = 0; y0 < g.h; y0 += 8)
        for (int x = 0; x < g.w; x += 8) {
            if (keep && keep[(y0 >> 3) * kw + (x >> 3)]) continue;
            const int ctb = (y0 >> g.lh) * cols + (x >> g.lw);
            const uint32_t b = nox ? nox[ctb] : 0u;
            int32_t *h = work.data() + (size_t)ctb * 2 * saostats::kSlots;
            auto ld_rec = [&](int y, int (&o)[10]) {
                const T *row = rec + (size_t)(y < 0 ? 0 : (y >= g.h ? g.h - 1 : y)) * pitch;
                for (int i = 0; i < 10; i++) {
                    const int xx = x - 1 + i;
                    o[i] = row[xx < 0 ? 0 : (xx >= g.w ? g.w - 1 : xx)];
                }
            };
            auto ld_org = [&](int y, int (&o)[8]) {
                const T *row = org + (size_t)y * pitch;
                for (int i = 0; i < 8; i++) o[i] = row[x + i < g.w ? x + i : g.w - 1];
            };
            auto add = [&](int slot, int d) {
                h[slot] += 1;
                h[saostats::kSlots + slot] += d;
            };
            if (saostats::needs_check(g, b, x, y0)) saostats::block<true>(g, b, x, y0, ld_rec, ld_org, add);
            else saostats::block<false>(g, b, x, y0, ld_rec, ld_org, add);
        }
    for (int c = 0; c < rows * cols; c++)
        for (int bin = 0; bin < saostats::kBins; bin++) out[(size_t)c * saostats::kBins + bin] = work[(size_t)c * 2 * saostats::kSlots + saostats::bin_slot(bin)];
}

int run_stats(const char *in, const char *outp)
{
    std::vector<uint8_t> buf;
    if (!read_all(in, buf) || buf.size() < 9 * sizeof(int32_t)) return 2;
    int32_t hd[9];
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int w = hd[0], h = hd[1], sb = hd[2], bd = hd[3], lw = hd[4], lh = hd[5], pitch = hd[8];
    const saostats::Geo g = {w, h, lw, lh, bd - 5};
    const int rows = (h + (1 << lh) - 1) >> lh, cols = (w + (1 << lw) - 1) >> lw, kh = (h + 7) / 8, kw = (w + 7) / 8;
    const size_t plane = (size_t)h * pitch * sb, nkeep = hd[6] ? (size_t)kh * kw : 0, nnox = hd[7] ? (size_t)rows * cols : 0;
    if (buf.size() != sizeof(hd) + 2 * plane + nkeep + nnox) return 3;
    /* every operand in a heap block of its own size */
    const uint8_t *p = buf.data() + sizeof(hd);
    std::vector<uint8_t> rec(p, p + plane), org(p + plane, p + 2 * plane), keep(p + 2 * plane, p + 2 * plane + nkeep),
        nox(p + 2 * plane + nkeep, p + 2 * plane + nkeep + nnox);
    std::vector<int32_t> out((size_t)rows * cols * saostats::kBins, 0);
    const uint8_t *k = hd[6] ? keep.data() : nullptr, *n = hd[7] ? nox.data() : nullptr;
    if (sb == 1) stats_plane<uint8_t>(rec.data(), org.data(), pitch, g, k, n, out.data());
    else stats_plane<uint16_t>(reinterpret_cast<const uint16_t *>(rec.data()), reinterpret_cast<const uint16_t *>(org.data()), pitch, g, k, n, out.data());
    return write_all(outp, out.data(), out.size() * sizeof(int32_t)) ? 0 : 4;
}

int run_pick(const char *in, const char *outp)
{
    std::vector<uint8_t> buf;
    if (!read_all(in, buf) || buf.size() < 4 * sizeof(int32_t)) return 2;
    int32_t hd[4];
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int bd = hd[0], n = hd[2], joint = hd[3];
    const long long lambda = hd[1];
    const size_t one = (size_t)n * saostats::kBins;
    if (buf.size() != sizeof(hd) + one * sizeof(int32_t) * (joint ? 2 : 1)) return 3;
    std::vector<int32_t> st(one * (joint ? 2 : 1));
    std::memcpy(st.data(), buf.data() + sizeof(hd), st.size() * sizeof(int32_t));
    const int M = (1 << ((bd < 10 ? bd : 10) - 5)) - 1;
    std::vector<uint8_t> out((size_t)n * 6 * (joint ? 2 : 1) + (size_t)n * 8);
    for (int i = 0; i < n; i++) {
        saostats::BinPick a[saostats::kPickBins], b[saostats::kPickBins];
        for (int k = 0; k < saostats::kPickBins; k++) {
            a[k] = saostats::pick_bin(st.data() + (size_t)i * saostats::kBins, k, M, lambda);
            if (joint) b[k] = saostats::pick_bin(st.data() + one + (size_t)i * saostats::kBins, k, M, lambda);
        }
        DbkSaoCtb pa, pb;
        const long long dd = saostats::pick_ctb(a, joint ? b : nullptr, lambda, pa, &pb);
        static_assert(sizeof(DbkSaoCtb) == 6, "hevcdbk_sao_ctb is six bytes");
        std::memcpy(out.data() + (size_t)i * 6, &pa, 6);
        if (joint) std::memcpy(out.data() + (size_t)(n + i) * 6, &pb, 6);
        std::memcpy(out.data() + (size_t)n * 6 * (joint ? 2 : 1) + (size_t)i * 8, &dd, 8);
    }
    return write_all(outp, out.data(), out.size()) ? 0 : 4;
}

} /* namespace */

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s stats|pick IN OUT\n", argv[0]);
        return 1;
    }
    if (!std::strcmp(argv[1], "stats")) return run_stats(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "pick")) return run_pick(argv[2], argv[3]);
    return 1;
}
