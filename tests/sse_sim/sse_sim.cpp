/*
 * sse_sim.cpp -- csrc/sse.h compiled for the CPU: a stand-alone program that runs what a wave of the SSE kernels does -- every lane's
 * block sums, then the butterfly STEP BY STEP over all 64 lanes, then the stores -- region by region over a plane, and the walk of
 * the totals kernel thread by thread.  tests/test_sse_cpu.py writes the operands into a file, runs the program -- plain and under
 * -fsanitize=address,undefined -- and compares what comes back with tests/sse_ref.py.  A plane lives in a heap block that ENDS with
 * the last sample of its last row (off + pitch * (h - 1) + a row of samples): a read behind it on any load path is the
 * sanitizer's to find, as is a load at an address its path may not assume.
 *
 *   sse_sim plane IN OUT    IN: int32 w, h, sample_bytes, lw, lh, pairs, mode (0 sample by sample, 1 four samples, 2 sixteen bytes),
 *                           acc64, rec_pitch, org_pitch, rec_off, org_off (bytes); then rec and org, each off + pitch * (h - 1) +
 *                           row bytes.  OUT: rows x cols uint64 (pairs: the even samples' grid, then the odd samples')
 *   sse_sim totals IN OUT   IN: int32 ctbs_x, ctbs_y, sse_stride, has_idx, idx_stride, n_slices; then (ctbs_y - 1) * stride + ctbs_x
 *                           uint64 and, if has_idx, as many uint16 by idx_stride.  OUT: n_slices uint64, then the frame total
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "sse.h"

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

struct Geo {
    int w, h, lw, lh;
    long long rec_pitch, org_pitch;
};

/* one instantiation of the kernel, wave by wave */
template <typename T, int MODE, bool ACC64, bool PAIRS>
void run_kernel(const uint8_t *rec, const uint8_t *org, const Geo &g, unsigned long long *even, unsigned long long *odd)
{
    constexpr int NS = PAIRS ? 16 : (MODE == sse::kWide ? 16 / (int)sizeof(T) : 8);
    constexpr int BW = PAIRS ? 8 : NS, BW_LOG2 = BW == 16 ? 4 : 3;
    constexpr int SPLIT = PAIRS ? sse::kParity : (NS == 16 ? sse::kHalves : sse::kOne);
    using Acc = typename std::conditional<ACC64, unsigned long long, uint32_t>::type;
    const int cols = (g.w + (1 << g.lw) - 1) >> g.lw;
    const int hs = sse::h_steps(g.lw, BW_LOG2), vs = sse::v_steps(g.lh);
    for (int ry = 0; ry < g.h; ry += 64)
        for (int rx = 0; rx < g.w + 8 * BW; rx += 8 * BW) { /* one region beyond the plane too: it must store nothing and read nothing */
            unsigned long long s[64][2], t[64][2];
            for (int lane = 0; lane < 64; lane++) {
                const sse::Block b = sse::block_of(rx, ry, lane, BW, g.w, g.h);
                sse::lane_sums<T, MODE, NS, SPLIT, Acc>(rec, org, g.rec_pitch, g.org_pitch, b, PAIRS ? 2 : 1, s[lane]);
                sse::fold<SPLIT>(g.lw, s[lane]);
            }
            for (int i = 0; i < hs + vs; i++) { /* a step of the butterfly: every lane adds its partner's value of BEFORE the step */
                const int mask = sse::step_mask(i, hs);
                for (int lane = 0; lane < 64; lane++)
                    for (int k = 0; k < 2; k++) t[lane][k] = s[lane][k] + s[lane ^ mask][k];
                std::memcpy(s, t, sizeof(s));
            }
            for (int lane = 0; lane < 64; lane++)
                sse::store_ctbs<SPLIT>(lane, rx, ry, BW, g.w, g.h, g.lw, g.lh, hs, vs, s[lane], [&](int which, int cx, int cy, unsigned long long v) {
                    unsigned long long *out = which ? odd : even;
                    if (out[(size_t)cy * cols + cx] != ~0ull) std::abort(); /* written twice */
                    out[(size_t)cy * cols + cx] = v;
                });
        }
}

template <typename T, bool PAIRS>
void run_any(int mode, bool acc64, const uint8_t *rec, const uint8_t *org, const Geo &g, unsigned long long *even, unsigned long long *odd)
{
    if (acc64) {
        if (mode == sse::kWide) run_kernel<T, sse::kWide, true, PAIRS>(rec, org, g, even, odd);
        else if (mode == sse::kQuad) run_kernel<T, sse::kQuad, true, PAIRS>(rec, org, g, even, odd);
        else run_kernel<T, sse::kScalar, true, PAIRS>(rec, org, g, even, odd);
    } else {
        if (mode == sse::kWide) run_kernel<T, sse::kWide, false, PAIRS>(rec, org, g, even, odd);
        else if (mode == sse::kQuad) run_kernel<T, sse::kQuad, false, PAIRS>(rec, org, g, even, odd);
        else run_kernel<T, sse::kScalar, false, PAIRS>(rec, org, g, even, odd);
    }
}

int run_plane(const char *in, const char *outp)
{
    std::vector<uint8_t> buf;
    int32_t hd[12];
    if (!read_all(in, buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int w = hd[0], h = hd[1], sb = hd[2], lw = hd[3], lh = hd[4], pairs = hd[5], mode = hd[6], acc64 = hd[7];
    const size_t rec_pitch = (size_t)hd[8], org_pitch = (size_t)hd[9], rec_off = (size_t)hd[10], org_off = (size_t)hd[11];
    const size_t row = (size_t)w * sb * (pairs ? 2 : 1);
    const size_t nrec = rec_off + rec_pitch * (h - 1) + row, norg = org_off + org_pitch * (h - 1) + row;
    if (buf.size() != sizeof(hd) + nrec + norg) return 3;
    /* heap blocks of exactly the operands' size (malloc: 16-byte aligned, so `off` decides the alignment of the plane) */
    uint8_t *rec = (uint8_t *)std::malloc(nrec), *org = (uint8_t *)std::malloc(norg);
    if (!rec || !org) return 5;
    std::memcpy(rec, buf.data() + sizeof(hd), nrec);
    std::memcpy(org, buf.data() + sizeof(hd) + nrec, norg);
    const int rows = (h + (1 << lh) - 1) >> lh, cols = (w + (1 << lw) - 1) >> lw;
    std::vector<unsigned long long> out((size_t)rows * cols * (pairs ? 2 : 1), ~0ull);
    const Geo g = {w, h, lw, lh, (long long)rec_pitch, (long long)org_pitch};
    unsigned long long *even = out.data(), *odd = out.data() + (size_t)rows * cols;
    if (sb == 1) {
        if (pairs) run_any<uint8_t, true>(mode, false, rec + rec_off, org + org_off, g, even, odd);
        else run_any<uint8_t, false>(mode, false, rec + rec_off, org + org_off, g, even, odd);
    } else {
        if (pairs) run_any<uint16_t, true>(mode, acc64 != 0, rec + rec_off, org + org_off, g, even, odd);
        else run_any<uint16_t, false>(mode, acc64 != 0, rec + rec_off, org + org_off, g, even, odd);
    }
    std::free(rec);
    std::free(org);
    return write_all(outp, out.data(), out.size() * sizeof(out[0])) ? 0 : 4;
}

int run_totals(const char *in, const char *outp)
{
    std::vector<uint8_t> buf;
    int32_t hd[6];
    if (!read_all(in, buf) || buf.size() < sizeof(hd)) return 2;
    std::memcpy(hd, buf.data(), sizeof(hd));
    const int cx = hd[0], cy = hd[1], stride = hd[2], has_idx = hd[3], istride = hd[4], n_slices = hd[5];
    const size_t nsse = (size_t)(cy - 1) * stride + cx, nidx = has_idx ? (size_t)(cy - 1) * istride + cx : 0;
    if (buf.size() != sizeof(hd) + nsse * 8 + nidx * 2 || n_slices < 1 || n_slices > sse::kMaxSlices) return 3;
    std::vector<unsigned long long> sse_in(nsse);
    std::vector<uint16_t> idx(nidx);
    std::memcpy(sse_in.data(), buf.data() + sizeof(hd), nsse * 8);
    if (nidx) std::memcpy(idx.data(), buf.data() + sizeof(hd) + nsse * 8, nidx * 2);
    std::vector<unsigned long long> tot((size_t)n_slices + 1, 0); /* the frame's array as the kernel keeps it in LDS; the frame total last */
    constexpr int kThreads = 1024;
    for (int tid = 0; tid < kThreads; tid++) {
        auto flush = [&](int slice, unsigned long long v) {
            if (slice < 0 || slice >= n_slices) std::abort();
            tot[(size_t)slice] += v;
        };
        tot[(size_t)n_slices] += sse::totals_walk(sse_in.data(), stride, has_idx ? idx.data() : nullptr, istride, cx, cy, n_slices, tid >> 6,
                                                  kThreads / 64, tid & 63, 64, flush);
    }
    return write_all(outp, tot.data(), tot.size() * 8) ? 0 : 4;
}

} /* namespace */

int main(int argc, char **argv)
{
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s plane|totals IN OUT\n", argv[0]);
        return 1;
    }
    if (!std::strcmp(argv[1], "plane")) return run_plane(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "totals")) return run_totals(argv[2], argv[3]);
    return 1;
}
