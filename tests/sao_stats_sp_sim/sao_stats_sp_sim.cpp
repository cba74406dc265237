/*
 * sao_stats_sp_sim.cpp -- csrc/sao_stats_sp.h and csrc/sao_stats.h compiled for the CPU: a stand-alone program that walks a plane of
 * interleaved Cb / Cr pairs as the kernel of sao_stats_sp.hip does -- region by region of 64 x 64 pairs, lane by lane (one 8 x 8
 * block of pairs each), component by component -- through the SAME loaders, in the wide form (four pairs per load) or sample by
 * sample.  tests/test_sao_stats_sp_cpu.py writes the operands into a file, runs the program -- plain and under
 * -fsanitize=address,undefined -- and compares what comes back with tests/sao_stats_sp_ref.py.  Every operand lives in a heap block
 * of exactly its size: a read outside it is the sanitizer's to find.
 *
 *   sao_stats_sp_sim IN OUT   IN: int32 w, h (pairs), sample_bytes, bit_depth, ctb_log2, has_keep, has_nox, pitch (samples, at least
 *                             2 w), wide, n_frames, org_shared; rec (n_frames x h rows of `pitch` samples), org (the same, or one
 *                             frame if org_shared), keep (n_frames x ceil(h/8) x ceil(w/8)), nox (n_frames x CTB rows x columns).
 *                             OUT: per frame 96 int32 per CTB of Cb, then the same of Cr
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sao_stats_sp.h"

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

/* the kernel's operands, on the host */
struct Args {
    const uint8_t *rec, *org;
    long long pitch, rec_frame_stride, org_frame_stride; /* bytes */
    const uint8_t *keep, *nox;
    int keep_stride, nox_stride;
    long long keep_frame_stride, nox_frame_stride;
};

template <typename T, bool VEC>
void stats_frame(const Args &a, const saostats::Geo &g, int f, int32_t *out_cb, int32_t *out_cr)
{
    const int lg = g.lw, cols = (g.w + (1 << lg) - 1) >> lg, rows = (g.h + (1 << lg) - 1) >> lg;
    std::vector<int32_t> work((size_t)2 * rows * cols * 2 * saostats::kSlots, 0); /* the working histograms, per component */
    const saostats_sp::Plane rec = saostats_sp::frame_of(a.rec, a.pitch, a.rec_frame_stride, f, g.w, g.h);
    const saostats_sp::Plane org = saostats_sp::frame_of(a.org, a.pitch, a.org_frame_stride, f, g.w, g.h);
    for (int ry = 0; ry < g.h; ry += 64)
        for (int rx = 0; rx < g.w; rx += 64)                /* a workgroup's region */
            for (int comp = 0; comp < 2; comp++)            /* its two waves */
                for (int lane = 0; lane < 64; lane++) {
                    const int x = rx + (lane & 7) * 8, y0 = ry + (lane >> 3) * 8;
                    if (x >= g.w || y0 >= g.h) continue;
                    if (a.keep && a.keep[saostats_sp::keep_at(x, y0, a.keep_stride, a.keep_frame_stride, f)]) continue;
                    const uint32_t b = a.nox ? a.nox[saostats_sp::nox_at(x, y0, lg, a.nox_stride, a.nox_frame_stride, f)] : 0u;
                    const int ctb = (y0 >> lg) * cols + (x >> lg);
                    int32_t *h = work.data() + ((size_t)comp * rows * cols + ctb) * 2 * saostats::kSlots;
                    auto ld_rec = [&](int y, int (&o)[10]) { saostats_sp::ld_rec<T, VEC>(rec, comp, x, y, o); };
                    auto ld_org = [&](int y, int (&o)[8]) { saostats_sp::ld_org<T, VEC>(org, comp, x, y, o); };
                    auto add = [&](int slot, int d) {
                        h[slot] += 1;
                        h[saostats::kSlots + slot] += d;
                    };
                    if (saostats::needs_check(g, b, x, y0)) saostats::block<true>(g, b, x, y0, ld_rec, ld_org, add);
                    else saostats::block<false>(g, b, x, y0, ld_rec, ld_org, add);
                }
    for (int comp = 0; comp < 2; comp++)
        for (int c = 0; c < rows * cols; c++)
            for (int bin = 0; bin < saostats::kBins; bin++)
                (comp ? out_cr : out_cb)[(size_t)c * saostats::kBins + bin] =
                    work[((size_t)comp * rows * cols + c) * 2 * saostats::kSlots + saostats::bin_slot(bin)];
}

int run(const char *in, const char *outp)
{
    std::vector<uint8_t> buf;
    int32_t hd[11];
    if (!read_all(in, buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int w = hd[0], h = hd[1], sb = hd[2], bd = hd[3], lg = hd[4], pitch = hd[7], wide = hd[8], n = hd[9], shared = hd[10];
    if (w < 8 || h < 8 || w % 4 || h % 4 || (sb != 1 && sb != 2) || lg < 3 || lg > 5 || pitch < 2 * w || n < 1) return 3;
    if (wide && pitch % 8 != 0) return 3; /* rows that start at a multiple of four pairs */
    const saostats::Geo g = {w, h, lg, lg, bd - 5};
    const int rows = (h + (1 << lg) - 1) >> lg, cols = (w + (1 << lg) - 1) >> lg, kh = (h + 7) / 8, kw = (w + 7) / 8;
    const size_t frame = (size_t)h * pitch * sb, nrec = frame * n, norg = frame * (shared ? 1 : n);
    const size_t nkeep = hd[5] ? (size_t)kh * kw * n : 0, nnox = hd[6] ? (size_t)rows * cols * n : 0;
    if (buf.size() != sizeof(hd) + nrec + norg + nkeep + nnox) return 3;
    /* every operand in a heap block of its own size */
    const uint8_t *p = buf.data() + sizeof(hd);
    std::vector<uint8_t> rec(p, p + nrec), org(p + nrec, p + nrec + norg), keep(p + nrec + norg, p + nrec + norg + nkeep),
        nox(p + nrec + norg + nkeep, p + nrec + norg + nkeep + nnox);
    const Args a = {rec.data(), org.data(), (long long)pitch * sb, (long long)frame, shared ? 0ll : (long long)frame,
                    hd[5] ? keep.data() : nullptr, hd[6] ? nox.data() : nullptr, kw, cols, (long long)kh * kw, (long long)rows * cols};
    const size_t grid = (size_t)rows * cols * saostats::kBins;
    std::vector<int32_t> out(grid * 2 * n, 0);
    for (int f = 0; f < n; f++) {
        int32_t *cb = out.data() + grid * 2 * f, *cr = cb + grid;
        if (sb == 1) wide ? stats_frame<uint8_t, true>(a, g, f, cb, cr) : stats_frame<uint8_t, false>(a, g, f, cb, cr);
        else wide ? stats_frame<uint16_t, true>(a, g, f, cb, cr) : stats_frame<uint16_t, false>(a, g, f, cb, cr);
    }
    return write_all(outp, out.data(), out.size() * sizeof(int32_t)) ? 0 : 4;
}

} /* namespace */

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 1;
    }
    return run(argv[1], argv[2]);
}
