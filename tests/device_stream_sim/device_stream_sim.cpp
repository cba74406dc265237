/*
 * device_stream_sim.cpp -- the device entries of csrc/deblock_host_h265.cpp and csrc/deblock_host_sp.cpp that share one of the
 * context's two scratch buffers (dev_tmp: the deblocked planes between the two launches of deblocking + SAO; dev_sao: the SAO
 * parameters and border bytes of 4:2:2 chroma planes rewritten for square CTBs) while the CALLER brings the streams.  The three
 * real host sources are linked against the model of the HIP runtime in tests/host_frame_sim/hip_model.cpp, which defers every
 * operation and decides what a kernel operation writes from what its operands hold when it RUNS.
 *
 *   device_stream_sim check SEED N     N sessions made from SEED; one line per violation (the first 100), the tallies -- calls per entry /
 *                                      scratch / scheduler, injected failures per entry / scratch / scheduler / kind, violations per property /
 *                                      scheduler / failing kind -- then "K violations"
 *
 * A session: one context, 1 to 3 caller streams (and in some sessions NULL, the context's compute stream), 2 to 8 calls, each an
 * entry with operands and device buffers of its own -- no two calls share a byte of caller memory, so the context's scratches are
 * all the calls have in common.  The inputs are written and drained before the first call; nothing synchronises with the host
 * until after the last.  What every call must have left in its dst is computed here from the operands it was given, with the
 * marker arithmetic of hip_model.h: SAO(deblock(src)), and for 4:2:2 chroma the grid doubled.
 *
 *   (A) every dst of every call that returned HEVCDBK_OK equals its expectation after the final drain
 *   (B) the model records no violation: bounds, memory kind, alignment, a wait whose record is on no stream, deadlock
 *   (C) the k-th launch / hipEventRecord / hipStreamWaitEvent / hipMalloc of the session fails: every OTHER call, queued earlier
 *       on another stream or made later, still meets (A) and (B) and returns HEVCDBK_OK; the failed call's dst is not looked at
 *   (D) a successful call that allocates nothing makes no blocking HIP call (hipStreamSynchronize, hipDeviceSynchronize,
 *       hipEventSynchronize); a call that grows a scratch may block
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/hevc_deblock.h"
#include "../host_frame_sim/hip_model.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
    bool coin() { return next() & 1; }
    bool pct(uint32_t p) { return below(100) < p; }
};

int g_violations = 0;
std::string g_session, g_run; /* g_run: scheduler/failing kind of the run in progress */
std::map<std::string, int> g_violations_by; /* property/scheduler/failing kind: every violation, printed or not */
void violation(const char *prop, const std::string &what)
{
    g_violations++;
    g_violations_by[std::string(prop) + "/" + g_run]++;
    if (g_violations <= 100) std::printf("violation (%s) %s: %s\n", prop, g_session.c_str(), what.c_str());
}

/* the entries.  Covered: every one that reaches through_scratch or sao_square_params (tests/test_device_stream_sim_cpu.py derives
 * the list from the sources); the last two touch no scratch and are mixed in */
enum Entry {
    E_REF_ONE, E_REF_PLANES, E_ONE0, E_PLANES0, E_SAO0, E_SAO_CF, E_SAO_NOX, E_SAO_G4, E_ONE_CF, E_ONE_NOX, E_ONE_SL, E_ONE_G4, E_PLANES_CF,
    E_PLANES_NOX, E_PLANES_SL, E_PLANES_G4, E_SP, E_SP_FUSED, E_NV12, N_COVERED, E_FILTER = N_COVERED, E_SAO_SP, N_ENTRIES
};
const char *const kEntry[N_ENTRIES] = {
    "hevc_deblock_sao_device", "hevc_deblock_sao_device_planes", "hevc_deblock_sao_h265_device", "hevc_deblock_sao_h265_device_planes",
    "hevc_sao_filter_device", "hevcdbk_sao_filter_device_cf", "hevcdbk_sao_filter_device_nox", "hevcdbk_sao_filter_device_g4",
    "hevcdbk_h265_deblock_sao_device_cf", "hevcdbk_h265_deblock_sao_device_nox", "hevcdbk_h265_deblock_sao_device_sl", "hevcdbk_h265_deblock_sao_device_g4",
    "hevcdbk_h265_deblock_sao_device_planes_cf", "hevcdbk_h265_deblock_sao_device_planes_nox", "hevcdbk_h265_deblock_sao_device_planes_sl",
    "hevcdbk_h265_deblock_sao_device_planes_g4", "hevcdbk_h265_deblock_sao_device_sp", "hevcdbk_h265_deblock_sao_device_sp_fused",
    "hevcdbk_h265_deblock_sao_device_nv12", "hevc_deblocking_filter_h265_device", "hevcdbk_sao_filter_device_sp"};
const char *const kSched[3] = {"eager", "lazy", "random"};
const char *const kScratch[4] = {"none", "tmp", "sao", "both"};
const int kFaultKinds[4] = {FAULT_LAUNCH, FAULT_EVENT_RECORD, FAULT_STREAM_WAIT_EVENT, FAULT_MALLOC};

bool is_sao_pass(int e) { return e == E_SAO0 || e == E_SAO_CF || e == E_SAO_NOX || e == E_SAO_G4 || e == E_SAO_SP; }
bool is_planes(int e) { return e == E_REF_PLANES || e == E_PLANES0 || (e >= E_PLANES_CF && e <= E_PLANES_G4); }
bool is_ref(int e) { return e == E_REF_ONE || e == E_REF_PLANES; }
bool takes_cf(int e) { return (e >= E_SAO_CF && e <= E_PLANES_G4); }
bool takes_g4(int e) { return e == E_SAO_G4 || e == E_ONE_G4 || e == E_PLANES_G4 || e == E_SP || e == E_SP_FUSED || e == E_NV12; }
bool takes_borders(int e) { return e == E_SAO_NOX || e == E_SAO_G4 || (e >= E_ONE_NOX && e <= E_ONE_G4) || (e >= E_PLANES_NOX && e <= E_NV12) || e == E_SAO_SP; }
bool takes_offsets(int e) { return e == E_ONE_SL || e == E_ONE_G4 || e == E_PLANES_SL || e == E_PLANES_G4 || e == E_SP || e == E_SP_FUSED || e == E_NV12; }
bool is_pairs_entry(int e) { return e == E_SP || e == E_SP_FUSED || e == E_SAO_SP; }

/* device memory of the model; every buffer an allocation of its own, so that the model's bounds are the buffer's */
std::vector<void *> g_bufs;
uint8_t *dev(size_t n)
{
    void *p = nullptr;
    if (hipMalloc(&p, n ? n : 1) != hipSuccess) { std::printf("out of memory\n"); std::exit(2); }
    g_bufs.push_back(p);
    return (uint8_t *)p;
}
uint8_t *dev_random(size_t n, Rng &r, unsigned mod)
{
    uint8_t *p = dev(n);
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(r.next() % mod);
    return p;
}
size_t span(size_t stride, size_t row, size_t rows) { return rows ? stride * (rows - 1) + row : 0; }

/* an operand array with rows and frames: what the model folds row by row */
struct Grid {
    const uint8_t *p = nullptr;
    size_t stride = 0, frame_stride = 0, row = 0, rows = 0; /* bytes */
    size_t bytes(unsigned frames) const { return (frame_stride ? frames - 1 : 0) * frame_stride + span(stride, row, rows); }
};
uint64_t fold_grid(uint64_t h, const Grid &g, unsigned frames)
{
    for (unsigned f = 0; f < (g.frame_stride ? frames : 1u); f++) h = model_fold_rows(h, g.p + f * g.frame_stride, g.stride, g.row, g.rows);
    return h;
}
/* one plane of a call */
struct PlaneOps {
    hevcdbk_device_planes p{};
    hevcdbk_sao_plane_cf sao{};
    const hevcdbk_sao_ctb *params_cr = nullptr;
    std::vector<uint8_t> in; /* src as it was written */
    size_t rb = 0, bytes = 0;
    int chroma = 0;          /* the plane model_m takes for the deblocking stage */
    bool dbk = false, sao_stage = false, rect = false;
    uint64_t hd = 0, hs = 0;
};

struct Call {
    int entry = 0, stream = -1, cf = 1, c_idx = 0, fused = 0;
    bool supports = false, borders = false, offsets = false, prm_null = false, qp_map = false;
    unsigned n_planes = 1, n_frames = 1, sb = 1, depth = 8, L = 4, W = 16, H = 16, qp = 30;
    hevcdbk_h265_params prm{0, 0, 0, 0};
    hevcdbk_sao_borders nox{};
    hevcdbk_h265_slice_offsets so{};
    PlaneOps pl[3];
    /* what the call is expected to use of the context */
    bool uses_tmp = false, uses_sao = false;
    size_t tmp_bytes = 0;            /* the largest request of dev_tmp */
    std::vector<size_t> tmp_needs;   /* every request, in the order of the planes */
    size_t sao_bytes = 0;            /* the one request of dev_sao: doubled parameters, then doubled border bytes, of every 4:2:2 plane */
    int scratch() const { return (uses_tmp ? 1 : 0) + (uses_sao ? 2 : 0); }
};

unsigned ceil_shift(unsigned v, unsigned s) { return (v + (1u << s) - 1) >> s; }
unsigned sub_w(int cf) { return cf == HEVCDBK_CHROMA_444 ? 1u : 2u; }
unsigned sub_h(int cf) { return cf == HEVCDBK_CHROMA_420 ? 2u : 1u; }

/* the choices of a call that need no memory: made once per session, the same for every run of it */
Call choose_call(Rng &r, int n_streams, bool use_null)
{
    Call c;
    c.entry = (int)r.below(N_ENTRIES);
    const int e = c.entry;
    const int pick = (int)r.below((uint32_t)(n_streams + (use_null ? 1 : 0)));
    c.stream = pick < n_streams ? pick : -1;
    c.sb = r.below(3) == 0 ? 2 : 1;
    c.depth = c.sb == 2 ? 10 : 8;
    c.n_frames = 1 + r.below(2);
    c.L = 4 + r.below(2);
    c.cf = takes_cf(e) ? (r.pct(50) ? HEVCDBK_CHROMA_422 : r.coin() ? HEVCDBK_CHROMA_420 : HEVCDBK_CHROMA_444) : HEVCDBK_CHROMA_420;
    /* luma sizes: mostly small, now and then the largest, so that sessions hold growth and a smaller request after a large one.
     * Entries that take planes in multiples of 4: luma in multiples of 8; else of 16, which keeps every chroma plane on the 8-sample grid */
    const unsigned step = takes_g4(e) ? 8 : 16, top = takes_g4(e) ? 136 : 128;
    auto dim = [&] { return r.pct(70) ? step * ((step == 16 ? 1 : 2) + r.below(3)) : r.pct(50) ? top : step * (2 + r.below(top / step - 1)); };
    c.W = dim();
    c.H = dim();
    c.n_planes = is_planes(e) ? (r.pct(70) ? 3 : 1 + r.below(2)) : 1;
    c.c_idx = is_planes(e) || e == E_NV12 ? 0 : (is_pairs_entry(e) ? 1 : (r.pct(30) ? 0 : 1 + (int)r.below(2)));
    c.qp = 20 + r.below(32);
    c.prm_null = r.pct(20);
    c.prm = {(int)r.below(13) - 6, (int)r.below(13) - 6, (int)r.below(25) - 12, (int)r.below(25) - 12};
    c.fused = r.pct(30) ? HEVCDBK_FUSED_OFF : HEVCDBK_FUSED_AUTO;
    c.supports = r.pct(35);
    c.borders = takes_borders(e) && r.coin();
    c.offsets = takes_offsets(e) && r.coin();
    c.qp_map = !is_ref(e) && !is_sao_pass(e) && r.pct(25);
    return c;
}

std::string describe(const Call &c)
{
    char b[256];
    std::snprintf(b, sizeof b, "%s luma=%ux%u cf=%d c_idx=%d planes=%u frames=%u sb=%u L=%u stream=%d fused=%d supports=%d nox=%d sl=%d map=%d scratch=%s", kEntry[c.entry], c.W,
                  c.H, c.cf, c.c_idx, c.n_planes, c.n_frames, c.sb, c.L, c.stream, c.fused, c.supports, c.borders, c.offsets, c.qp_map, kScratch[c.scratch()]);
    return b;
}

/* the 4:2:2 rewriting as the model's launchers do it: a hash of the caller's grid of every frame over the whole doubled grid */
Grid doubled(const Grid &g, size_t square_rows, unsigned frames, std::vector<uint8_t> &store)
{
    uint64_t h = kModelDeriveHash0;
    const unsigned nf = g.frame_stride ? frames : 1u;
    for (unsigned f = 0; f < nf; f++) h = model_fold(h, g.p + f * g.frame_stride, span(g.stride, g.row, g.rows));
    store.resize(nf * square_rows * g.row);
    model_derived(h, store.data(), store.size());
    Grid out;
    out.p = store.data();
    out.stride = out.row = g.row;
    out.rows = square_rows;
    out.frame_stride = g.frame_stride ? square_rows * g.row : 0;
    return out;
}

/* the buffers of a call, its operand structs, and the hashes its kernel operations must arrive at */
void build_call(Call &c, Rng &r)
{
    const int e = c.entry;
    const unsigned nf = c.n_frames, sb = c.sb;
    const int max_v = (1 << c.depth) - 1;
    const unsigned cols_l = ceil_shift(c.W, c.L), rows_l = ceil_shift(c.H, c.L);
    /* one operand of each kind for the picture */
    Grid nox, sl, map;
    if (c.borders) {
        nox.row = cols_l; nox.rows = rows_l; nox.stride = cols_l + r.below(2); nox.frame_stride = r.coin() ? 0 : nox.stride * rows_l;
        nox.p = dev_random(nox.bytes(nf), r, 256);
        c.nox = {nox.p, (unsigned)nox.stride, nox.frame_stride};
    }
    if (c.offsets) {
        const unsigned stride = cols_l + r.below(2);
        sl.row = sl.stride = 2 * (size_t)stride * rows_l; sl.rows = 1; sl.frame_stride = r.coin() ? 0 : sl.row;
        sl.p = dev_random(sl.bytes(nf), r, 256);
        c.so = {(const int8_t *)sl.p, stride, sl.frame_stride, c.L};
    }
    if (c.qp_map) {
        map.stride = cols_l + r.below(2); map.rows = rows_l; map.row = map.stride * rows_l;
        map.p = dev_random(map.row, r, 52);
    }
    const unsigned *tc = hevcdbk_default_tc_table(), *beta = hevcdbk_default_beta_table();
    const bool pairs = is_pairs_entry(e);
    const unsigned n = e == E_NV12 ? 2 : c.n_planes;
    const bool two_launch = !is_sao_pass(e) && e != E_FILTER && (e == E_SP || !c.supports || c.fused == HEVCDBK_FUSED_OFF);
    for (unsigned i = 0; i < n; i++) {
        PlaneOps &o = c.pl[i];
        const int idx = n > 1 ? (int)i : c.c_idx; /* 0 luma, 1 Cb, 2 Cr */
        const bool pair_plane = pairs || (e == E_NV12 && i == 1);
        const bool chroma = idx != 0;
        const unsigned w = chroma ? c.W / sub_w(c.cf) : c.W, h = chroma ? c.H / sub_h(c.cf) : c.H;
        const unsigned lw = chroma && sub_w(c.cf) == 2 ? c.L - 1 : c.L, lh = chroma && sub_h(c.cf) == 2 ? c.L - 1 : c.L;
        o.rect = lh != lw;
        o.chroma = chroma ? 1 : 0;
        o.dbk = !is_sao_pass(e);
        o.sao_stage = e != E_FILTER;
        o.rb = (size_t)w * sb * (pair_plane ? 2 : 1);
        hevcdbk_device_planes &p = o.p;
        p.pitch = o.rb + (r.below(3) == 0 ? 16 * sb : 0);
        p.frame_stride = p.pitch * h + (r.below(4) == 0 ? 2 * p.pitch : 0);
        p.n_frames = nf; p.plane_w = w; p.plane_h = h; p.bit_depth = c.depth; p.sample_bytes = sb; p.is_chroma = chroma;
        o.bytes = p.frame_stride * (nf - 1) + p.pitch * h;
        o.in.resize(o.bytes);
        for (auto &b : o.in) b = (uint8_t)r.next();
        uint8_t *src = dev(o.bytes), *dst = dev(o.bytes);
        std::memcpy(src, o.in.data(), o.bytes);
        std::memset(dst, 0xEE, o.bytes);
        p.src = src; p.dst = dst;
        if (two_launch) {
            c.uses_tmp = true;
            c.tmp_needs.push_back(o.bytes);
            if (o.bytes > c.tmp_bytes) c.tmp_bytes = o.bytes;
        }
        /* deblocking operands and hash */
        if (o.dbk) {
            const size_t nv = is_ref(e) ? hevcdbk_num_vert_bs(w, h) : hevcdbk_h265_num_vert_bs(w, h);
            const size_t nh = is_ref(e) ? hevcdbk_num_hor_bs(w, h) : hevcdbk_h265_num_hor_bs(w, h);
            p.vert_bs = dev_random(nv, r, 3);
            p.hor_bs = dev_random(nh, r, 3);
            uint64_t hh;
            if (is_ref(e)) {
                uint8_t tc8[52], beta8[52];
                for (int k = 0; k < 52; k++) { tc8[k] = (uint8_t)tc[k]; beta8[k] = (uint8_t)beta[k]; }
                const unsigned q = c.qp > 51 ? 51 : c.qp, shift = c.depth - 8;
                hh = kModelHash0;
                hh = model_fold(hh, tc8, 52);
                hh = model_fold(hh, beta8, 52);
                hh = model_fold_int(hh, (int)(tc[q] << shift));
                hh = model_fold_int(hh, (int)(beta[q] << shift));
                hh = model_fold_int(hh, max_v);
            } else {
                if (c.qp_map) { p.qp_map = map.p; p.qp_map_stride = (unsigned)map.stride; p.ctu_log2 = c.L; }
                const hevcdbk_h265_params zero = {0, 0, 0, 0}, &prm = c.prm_null ? zero : c.prm;
                hh = kModelHash0 ^ 0x265;
                hh = model_fold_int(hh, (int)(c.qp > 51 ? 51 : c.qp));
                /* with the per-slice operand the call's own pair is not an operand of the kernels */
                hh = model_fold_int(hh, c.offsets ? 0 : prm.tc_offset_div2 * 2);
                hh = model_fold_int(hh, c.offsets ? 0 : prm.beta_offset_div2 * 2);
                hh = model_fold_int(hh, idx == 1 ? prm.cb_qp_offset : idx == 2 ? prm.cr_qp_offset : 0);
                hh = model_fold_int(hh, max_v);
                if (c.qp_map) { hh = model_fold_int(hh, (int)map.stride); hh = model_fold_int(hh, (int)c.L); }
                if (pair_plane) hh = model_fold_int(hh, prm.cr_qp_offset);
            }
            hh = model_fold(hh, p.vert_bs, nv);
            hh = model_fold(hh, p.hor_bs, nh);
            if (c.qp_map && !is_ref(e)) hh = model_fold(hh, map.p, map.row);
            if (c.offsets) hh = fold_grid(hh, sl, nf);
            o.hd = hh;
        }
        /* SAO operands and hash */
        if (o.sao_stage) {
            const unsigned cols = ceil_shift(w, lw), sq_rows = ceil_shift(h, lw), src_rows = ceil_shift(h, lh);
            const size_t es = sizeof(hevcdbk_sao_ctb);
            Grid prm_g, cr_g, keep_g;
            const unsigned pstride = cols + r.below(2);
            prm_g.row = cols * es; prm_g.rows = src_rows; prm_g.stride = pstride * es; prm_g.frame_stride = r.coin() ? 0 : (size_t)pstride * src_rows * es;
            prm_g.p = dev_random(prm_g.bytes(nf), r, 256);
            o.sao = {(const hevcdbk_sao_ctb *)prm_g.p, pstride, prm_g.frame_stride / es, lw, lh, nullptr, 0, 0};
            if (pair_plane) {
                cr_g = prm_g;
                cr_g.p = dev_random(cr_g.bytes(nf), r, 256);
                o.params_cr = (const hevcdbk_sao_ctb *)cr_g.p;
            }
            if (r.coin()) {
                keep_g.row = (w + 7) / 8; keep_g.rows = (h + 7) / 8; keep_g.stride = keep_g.row + r.below(2);
                keep_g.frame_stride = r.coin() ? 0 : keep_g.stride * keep_g.rows;
                keep_g.p = dev_random(keep_g.bytes(nf), r, 2);
                o.sao.keep = keep_g.p; o.sao.keep_stride = (unsigned)keep_g.stride; o.sao.keep_frame_stride = keep_g.frame_stride;
            }
            std::vector<uint8_t> prm2, nox2;
            Grid prm_k = prm_g, nox_k = nox;
            nox_k.row = cols; nox_k.rows = src_rows;
            if (o.rect) {
                c.uses_sao = true;
                c.sao_bytes += (size_t)cols * sq_rows * (prm_g.frame_stride ? nf : 1u) * es + (c.borders ? (size_t)cols * sq_rows * (nox.frame_stride ? nf : 1u) : 0);
                prm_k = doubled(prm_g, sq_rows, nf, prm2);
                if (c.borders) nox_k = doubled(nox_k, sq_rows, nf, nox2);
            }
            uint64_t hh = model_sao_hash0(max_v, (int)c.depth - 5, (int)lw);
            hh = fold_grid(hh, prm_k, nf);
            if (pair_plane) hh = fold_grid(hh, cr_g, nf);
            if (o.sao.keep) hh = fold_grid(hh, keep_g, nf);
            if (c.borders) hh = fold_grid(hh, nox_k, nf);
            o.hs = hh;
        }
    }
}

int call_entry(hevcdbk_context *ctx, const Call &c, void *stream)
{
    const PlaneOps &o = c.pl[0];
    const hevcdbk_device_planes *p = &o.p;
    const hevcdbk_sao_plane_cf &s = o.sao;
    const hevcdbk_h265_params *prm = c.prm_null ? nullptr : &c.prm;
    const hevcdbk_sao_borders *b = c.borders ? &c.nox : nullptr;
    const hevcdbk_h265_slice_offsets *sl = c.offsets ? &c.so : nullptr;
    hevcdbk_device_planes pl[3];
    hevcdbk_sao_plane_cf cf[3];
    hevcdbk_sao_plane sq[3];
    for (int i = 0; i < 3; i++) {
        pl[i] = c.pl[i].p;
        cf[i] = c.pl[i].sao;
        sq[i] = {cf[i].params, cf[i].params_stride, cf[i].params_frame_stride, cf[i].ctb_log2_w, cf[i].keep, cf[i].keep_stride, cf[i].keep_frame_stride};
    }
#define SAO_SQ s.params, s.params_stride, s.params_frame_stride, s.ctb_log2_w, s.keep, s.keep_stride, s.keep_frame_stride
#define SAO_CF s.params, s.params_stride, s.params_frame_stride, s.ctb_log2_w, s.ctb_log2_h, s.keep, s.keep_stride, s.keep_frame_stride
#define SAO_SP s.params, o.params_cr, s.params_stride, s.params_frame_stride, s.ctb_log2_w, s.keep, s.keep_stride, s.keep_frame_stride
    switch (c.entry) {
    case E_REF_ONE: return hevc_deblock_sao_device(ctx, p, c.qp, nullptr, SAO_SQ, c.fused, stream);
    case E_REF_PLANES: return hevc_deblock_sao_device_planes(ctx, pl, c.n_planes, c.qp, nullptr, sq, c.fused, stream);
    case E_ONE0: return hevc_deblock_sao_h265_device(ctx, p, c.c_idx, c.qp, prm, SAO_SQ, c.fused, stream);
    case E_PLANES0: return hevc_deblock_sao_h265_device_planes(ctx, pl, c.n_planes, c.qp, prm, sq, c.fused, stream);
    case E_SAO0: return hevc_sao_filter_device(ctx, p, SAO_SQ, stream);
    case E_SAO_CF: return hevcdbk_sao_filter_device_cf(ctx, p, SAO_CF, stream);
    case E_SAO_NOX: return hevcdbk_sao_filter_device_nox(ctx, p, SAO_CF, b, stream);
    case E_SAO_G4: return hevcdbk_sao_filter_device_g4(ctx, p, SAO_CF, b, stream);
    case E_ONE_CF: return hevcdbk_h265_deblock_sao_device_cf(ctx, p, c.c_idx, c.cf, c.qp, prm, SAO_CF, c.fused, stream);
    case E_ONE_NOX: return hevcdbk_h265_deblock_sao_device_nox(ctx, p, c.c_idx, c.cf, c.qp, prm, SAO_CF, c.fused, b, stream);
    case E_ONE_SL: return hevcdbk_h265_deblock_sao_device_sl(ctx, p, c.c_idx, c.cf, c.qp, prm, SAO_CF, c.fused, b, sl, stream);
    case E_ONE_G4: return hevcdbk_h265_deblock_sao_device_g4(ctx, p, c.c_idx, c.cf, c.qp, prm, SAO_CF, c.fused, b, sl, stream);
    case E_PLANES_CF: return hevcdbk_h265_deblock_sao_device_planes_cf(ctx, pl, c.n_planes, c.cf, c.qp, prm, cf, c.fused, stream);
    case E_PLANES_NOX: return hevcdbk_h265_deblock_sao_device_planes_nox(ctx, pl, c.n_planes, c.cf, c.qp, prm, cf, c.fused, b, stream);
    case E_PLANES_SL: return hevcdbk_h265_deblock_sao_device_planes_sl(ctx, pl, c.n_planes, c.cf, c.qp, prm, cf, c.fused, b, sl, stream);
    case E_PLANES_G4: return hevcdbk_h265_deblock_sao_device_planes_g4(ctx, pl, c.n_planes, c.cf, c.qp, prm, cf, c.fused, b, sl, stream);
    case E_SP: return hevcdbk_h265_deblock_sao_device_sp(ctx, p, c.qp, prm, SAO_SP, c.fused, b, sl, stream);
    case E_SP_FUSED: return hevcdbk_h265_deblock_sao_device_sp_fused(ctx, p, c.qp, prm, SAO_SP, c.fused, b, sl, stream);
    case E_NV12: {
        const hevcdbk_sao_plane_cf &s1 = c.pl[1].sao;
        const hevcdbk_sao_plane_sp sp = {s1.params, c.pl[1].params_cr, s1.params_stride, s1.params_frame_stride, s1.ctb_log2_w, s1.keep, s1.keep_stride, s1.keep_frame_stride};
        return hevcdbk_h265_deblock_sao_device_nv12(ctx, &pl[0], &pl[1], c.qp, prm, &cf[0], &sp, c.fused, b, sl, stream);
    }
    case E_FILTER: return hevc_deblocking_filter_h265_device(ctx, p, c.c_idx, c.qp, prm, HEVCDBK_KERNEL_AUTO, stream);
    default: return hevcdbk_sao_filter_device_sp(ctx, p, SAO_SP, b, stream);
    }
}

/* (A): every sample of every frame; -1 = right, else the first wrong row */
long first_wrong_row(const PlaneOps &o)
{
    const hevcdbk_device_planes &p = o.p;
    const uint8_t *dst = (const uint8_t *)p.dst;
    for (unsigned f = 0; f < p.n_frames; f++)
        for (unsigned y = 0; y < p.plane_h; y++) {
            const size_t at = f * p.frame_stride + y * p.pitch;
            for (size_t x = 0; x < o.rb; x++) {
                uint8_t want = o.in[at + x];
                if (o.dbk) want ^= model_m(o.hd, o.chroma, y, (unsigned)x);
                if (o.sao_stage) want ^= model_m(o.hs, kModelSaoPlane, y, (unsigned)x);
                if (dst[at + x] != want) return (long)(f * p.plane_h + y);
            }
        }
    return -1;
}

struct Session {
    uint32_t seed;
    int sched, n_streams;
    bool use_null;
    std::vector<Call> calls; /* the choices; the buffers are built per run */
};

/* what a run reports of each call */
struct CallReport {
    int rc = 0, hip_calls[FAULT_KINDS][2] = {}, blocking = 0, frees = 0;
};

struct Tally {
    std::map<std::string, int> ran, faults, schedulers, counts;
} g_tally;

/* one run of the session; fault_kind 0: the fault-free run */
std::vector<CallReport> run(const Session &s, int fault_kind, int fault_at, const Rng &r_data)
{
    Rng r = r_data;
    char when[64];
    std::snprintf(when, sizeof when, fault_kind ? "%s #%d fails" : "fault-free", model_fault_name(fault_kind), fault_at);
    g_run = std::string(kSched[s.sched]) + "/" + model_fault_name(fault_kind);
    ModelCase quiet;
    model_begin(quiet); /* the set-up below is not the code under test */
    hevcdbk_context *ctx = nullptr;
    if (hevcdbk_create(0, &ctx) != HEVCDBK_OK) { std::printf("hevcdbk_create failed\n"); std::exit(2); }
    std::vector<hipStream_t> streams((size_t)s.n_streams);
    for (hipStream_t &st : streams) (void)hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    std::vector<Call> calls = s.calls;
    for (Call &c : calls) build_call(c, r);
    model_drain();
    ModelCase mc;
    mc.sched = s.sched;
    mc.seed = s.seed * 977u + 1;
    mc.fault_kind = fault_kind;
    mc.fault_at = fault_at;
    model_begin(mc);
    std::vector<CallReport> rep(calls.size());
    for (size_t i = 0; i < calls.size(); i++) {
        const Call &c = calls[i];
        CallReport &cr = rep[i];
        for (int k = 0; k < FAULT_KINDS; k++) cr.hip_calls[k][0] = model_calls(k);
        const int b0 = model_blocking_calls(), f0 = model_device_frees();
        model_set_supports(c.supports);
        cr.rc = call_entry(ctx, c, c.stream < 0 ? nullptr : (void *)streams[(size_t)c.stream]);
        for (int k = 0; k < FAULT_KINDS; k++) cr.hip_calls[k][1] = model_calls(k);
        cr.blocking = model_blocking_calls() - b0;
        cr.frees = model_device_frees() - f0;
        const bool hit = fault_kind && cr.hip_calls[fault_kind][0] < fault_at && cr.hip_calls[fault_kind][1] >= fault_at;
        const std::string what = std::string(when) + ": call " + std::to_string(i) + " " + describe(c);
        if (hit) {
            g_tally.faults[std::string(kEntry[c.entry]) + "/" + kScratch[c.scratch()] + "/" + kSched[s.sched] + "/" + model_fault_name(fault_kind)]++;
            if (cr.rc == HEVCDBK_OK) violation("C", what + ": returned HEVCDBK_OK although a HIP call inside it failed");
        } else if (cr.rc != HEVCDBK_OK)
            violation(fault_kind ? "C" : "A", what + ": returned " + std::to_string(cr.rc) + " (" + hevcdbk_last_error(ctx) + ")");
        /* (D) */
        if (cr.rc == HEVCDBK_OK && cr.blocking && cr.hip_calls[FAULT_MALLOC][1] == cr.hip_calls[FAULT_MALLOC][0])
            violation("D", what + ": " + std::to_string(cr.blocking) + " blocking HIP calls in a call that allocated nothing");
    }
    model_drain();
    for (const std::string &v : model_violations()) violation("B", std::string(when) + ": " + v);
    for (size_t i = 0; i < calls.size(); i++) {
        if (rep[i].rc != HEVCDBK_OK) continue;
        const Call &c = calls[i];
        for (unsigned k = 0; k < (c.entry == E_NV12 ? 2u : c.n_planes); k++) {
            const long row = first_wrong_row(c.pl[k]);
            if (row >= 0) violation(fault_kind ? "C" : "A", std::string(when) + ": call " + std::to_string(i) + " " + describe(c) + ": plane " + std::to_string(k) + " is wrong from row " + std::to_string(row));
        }
    }
    for (hipStream_t st : streams) (void)hipStreamDestroy(st);
    hevcdbk_destroy(ctx);
    for (void *p : g_bufs) (void)hipFree(p);
    g_bufs.clear();
    return rep;
}

void run_session(uint32_t seed)
{
    Rng r{0x51ed270b1ull * (seed + 1)};
    Session s;
    s.seed = seed;
    s.sched = (int)r.below(3);
    s.n_streams = r.pct(5) ? 1 : 2 + (int)r.below(2);
    s.use_null = r.pct(30);
    const unsigned n_calls = 2 + r.below(7);
    for (unsigned i = 0; i < n_calls; i++) s.calls.push_back(choose_call(r, s.n_streams, s.use_null));
    /* in more than half of the sessions the first call is the largest there is: every later request of a scratch is the smaller one
     * after a large one, and no later call has a reason to block */
    if (r.pct(60)) {
        Call &c = s.calls[0];
        c.W = c.H = takes_g4(c.entry) ? 136 : 128;
        c.n_frames = 2;
        c.sb = 2;
        c.depth = 10;
    }
    g_session = "seed=" + std::to_string(seed) + " sched=" + kSched[s.sched] + " streams=" + std::to_string(s.n_streams) + (s.use_null ? "+NULL" : "") +
                " calls=" + std::to_string(n_calls);
    const Rng r_data = r;

    const std::vector<CallReport> rep = run(s, FAULT_NONE, 0, r_data);
    /* the session's tallies, from the fault-free run.  The scratch a call uses is known from its operands (build_call); the
     * expectation is tied to the code under test by the context's allocations: a request of dev_tmp or dev_sao that is the
     * scratch's first, or larger than every one before, allocates, and the entries allocate nothing else */
    std::vector<Call> calls = s.calls;
    {
        Rng rr = r_data;
        ModelCase quiet;
        model_begin(quiet);
        for (Call &c : calls) build_call(c, rr);
        for (void *p : g_bufs) (void)hipFree(p);
        g_bufs.clear();
    }
    g_tally.counts["sessions"]++;
    g_tally.schedulers[kSched[s.sched]]++;
    bool contended = false, grew = false, shrank = false, first[2] = {false, false};
    int last_stream[2] = {-2, -2}, blocked_since[2] = {0, 0};
    size_t tmp_cap = 0, tmp_now = 0, sao_now = 0;
    g_run = std::string(kSched[s.sched]) + "/" + model_fault_name(FAULT_NONE);
    for (size_t i = 0; i < calls.size(); i++) {
        const Call &c = calls[i];
        g_tally.ran[std::string(kEntry[c.entry]) + "/" + kScratch[c.scratch()] + "/" + kSched[s.sched]]++;
        for (int k = 0; k < 2; k++) {
            blocked_since[k] += rep[i].blocking;
            if (!(k == 0 ? c.uses_tmp : c.uses_sao)) continue;
            if (last_stream[k] == -2) first[k] = true;
            else if (last_stream[k] != c.stream && blocked_since[k] == 0) contended = true;
            last_stream[k] = c.stream;
            blocked_since[k] = 0;
        }
        if (rep[i].frees) grew = true;
        if (c.uses_tmp) {
            if (c.tmp_bytes < tmp_cap) shrank = true;
            if (c.tmp_bytes > tmp_cap) tmp_cap = c.tmp_bytes;
        }
        int allocations = 0;
        for (size_t need : c.tmp_needs)
            if (need > tmp_now) { tmp_now = need; allocations++; }
        if (c.sao_bytes > sao_now) { sao_now = c.sao_bytes; allocations++; }
        const int made = rep[i].hip_calls[FAULT_MALLOC][1] - rep[i].hip_calls[FAULT_MALLOC][0];
        if (made != allocations)
            violation("A", "call " + std::to_string(i) + " " + describe(c) + ": " + std::to_string(made) + " allocations, " + std::to_string(allocations) +
                               " expected of a call that asks dev_tmp for up to " + std::to_string(c.tmp_bytes) + " and dev_sao for " + std::to_string(c.sao_bytes) + " bytes");
    }
    if (contended) g_tally.counts["contended"]++;
    if (grew) g_tally.counts["grew"]++;
    if (shrank) g_tally.counts["smaller_after_larger"]++;
    if (first[0]) g_tally.counts["first_use_tmp"]++;
    if (first[1]) g_tally.counts["first_use_sao"]++;

    /* (C): up to ten failures per session, each a run of its own; of all the HIP calls that can fail, the ones whose
     * (entry, scratch, kind, how many of the kind the call had made before) has been hit least so far -- scratch users first --
     * so that every kind reaches every site, at its first launch as well as at its last */
    struct Cand { int kind, at; std::string cell; bool scratch; };
    std::vector<Cand> cands;
    for (size_t i = 0; i < calls.size(); i++)
        for (int kind : kFaultKinds)
            for (int at = rep[i].hip_calls[kind][0] + 1; at <= rep[i].hip_calls[kind][1]; at++)
                cands.push_back({kind, at, std::string(kEntry[calls[i].entry]) + "/" + kScratch[calls[i].scratch()] + "/" + model_fault_name(kind) + "/" +
                                               std::to_string(at - rep[i].hip_calls[kind][0]), calls[i].scratch() != 0});
    static std::map<std::string, int> planned;
    for (int n = 0; n < 10 && !cands.empty(); n++) {
        size_t best = 0;
        long best_score = -1;
        for (size_t k = 0; k < cands.size(); k++) {
            const long score = (cands[k].scratch ? 1000000 : 0) + 1000 * (999 - (planned[cands[k].cell] > 999 ? 999 : planned[cands[k].cell])) + (long)r.below(1000);
            if (score > best_score) { best_score = score; best = k; }
        }
        const Cand c = cands[best];
        cands.erase(cands.begin() + (long)best);
        planned[c.cell]++;
        run(s, c.kind, c.at, r_data);
    }
}

int cmd_check(uint32_t seed, int n)
{
    for (int i = 0; i < n; i++) run_session(seed * 100003u + (uint32_t)i);
    for (auto &kv : g_tally.ran) std::printf("ran %s %d\n", kv.first.c_str(), kv.second);
    for (auto &kv : g_tally.schedulers) std::printf("scheduler %s %d\n", kv.first.c_str(), kv.second);
    for (auto &kv : g_tally.faults) std::printf("fault %s %d\n", kv.first.c_str(), kv.second);
    for (auto &kv : g_tally.counts) std::printf("count %s %d\n", kv.first.c_str(), kv.second);
    for (auto &kv : g_violations_by) std::printf("violations_by %s %d\n", kv.first.c_str(), kv.second);
    std::printf("%d violations\n", g_violations);
    return g_violations ? 1 : 0;
}

} /* namespace */

int main(int argc, char **argv)
{
    std::setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc == 4 && !std::strcmp(argv[1], "check")) return cmd_check((uint32_t)std::strtoul(argv[2], nullptr, 10), std::atoi(argv[3]));
    std::fprintf(stderr, "usage: device_stream_sim check SEED N\n");
    return 2;
}
