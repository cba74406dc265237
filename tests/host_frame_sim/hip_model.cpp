/*
 * hip_model.cpp -- the model of hip_model.h: the 31 HIP symbols the host sources use, and the kernel launchers and predicates
 * of deblock_kernels.h.  Only the thread inside a host entry makes HIP calls (the staging crew never does), so the model needs no
 * lock of its own.  A launcher enqueues a marker operation; see run_marker(), run_sao(), run_fused() and run_derive() for what
 * they do when they execute.
 */
#include <hip/hip_runtime_api.h>

#include <sys/mman.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>

#include "../../gpu_video_codec_amd/csrc/deblock_kernels.h"
#include "hip_model.h"

#ifdef HEVCDBK_DIAG
DbkDiag g_dbk_diag; /* the diagnostic build's knobs live in the kernel translation unit */
#endif

namespace {

enum Kind { DEVICE, FINE, PINNED, REGISTERED, UNMAPPED };
struct Alloc {
    char *host; /* the address the host uses (DEVICE: the model's own backing) */
    char *dev;  /* the address a kernel or a DMA's device side uses */
    size_t n;
    Kind kind;
};
struct Region { char *primary, *alias; size_t n; int fd; };

struct Event {
    uint64_t recorded = 0, completed = 0; /* generation of the last record enqueued / the latest one executed */
    int not_ready_left = 0;
    /* per record: a wait is for ONE record, and the records of an event that several streams record need not execute in order */
    std::vector<bool> done{true};
    bool is_done(uint64_t gen) const { return gen < done.size() && done[gen]; }
    void mark(uint64_t gen)
    {
        if (done.size() <= gen) done.resize(gen + 1, false);
        done[gen] = true;
        if (completed < gen) completed = gen;
    }
};
struct Op {
    enum { WORK, RECORD, WAIT } kind;
    std::function<void()> fn;
    Event *ev = nullptr;
    uint64_t gen = 0;
    std::string what;
};
struct Stream { std::deque<Op> q; };

struct Model {
    ModelCase c;
    uint64_t rng = 1;
    std::vector<Alloc> allocs;
    std::vector<Region> regions;
    std::vector<Stream *> streams;
    std::vector<Event *> events;
    int calls[FAULT_KINDS] = {};
    std::vector<std::string> violations;
    std::vector<ModelWrite> writes;
    int sync_pageable = 0;
    int blocking = 0, frees = 0;
    int depth = 0;
} M;

thread_local hipEvent_t t_start = nullptr, t_stop = nullptr;

uint32_t rnd()
{
    M.rng = M.rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(M.rng >> 33);
}
void violation(const std::string &s)
{
    if (M.violations.size() < 64) M.violations.push_back(s);
}
bool fault(int kind)
{
    return ++M.calls[kind] == M.c.fault_at && M.c.fault_kind == kind;
}

/* [p, p + n) as a device-side address range: inside ONE allocation, of a kind a kernel or a DMA engine may touch */
bool dev_ok(const void *p, size_t n, const std::string &what)
{
    const char *c = (const char *)p;
    for (const Alloc &a : M.allocs) {
        if (a.kind == UNMAPPED || c < a.dev || c >= a.dev + a.n) continue;
        if (c + n > a.dev + a.n) {
            violation(what + ": runs " + std::to_string((size_t)(c + n - (a.dev + a.n))) + " bytes past the end of its allocation");
            return false;
        }
        return true;
    }
    for (const Alloc &a : M.allocs)
        if (a.kind == REGISTERED && c >= a.host && c < a.host + a.n) {
            violation(what + ": the HOST address of a registered range, not its devicePointer");
            return false;
        }
    violation(what + ": not device, page-locked or registered memory");
    return false;
}
/* the host side of an async copy: page-locked or registered throughout */
bool host_locked(const void *p, size_t n)
{
    const char *c = (const char *)p;
    for (const Alloc &a : M.allocs)
        if ((a.kind == PINNED || a.kind == REGISTERED) && c >= a.host && c + n <= a.host + a.n) return true;
    return false;
}

bool runnable(const Stream &s) { return !s.q.empty() && !(s.q.front().kind == Op::WAIT && !s.q.front().ev->is_done(s.q.front().gen)); }
void run_head(Stream &s)
{
    Op op = std::move(s.q.front());
    s.q.pop_front();
    if (op.kind == Op::WORK) op.fn();
    else if (op.kind == Op::RECORD) op.ev->mark(op.gen);
}
void force_event(Event *e, uint64_t gen);
/* run the stream's operations up to and including its n-th */
void force_ops(Stream &s, size_t n)
{
    if (++M.depth > 64) {
        violation("deadlock: a cycle of event waits");
        M.depth--;
        return;
    }
    for (size_t i = 0; i < n && !s.q.empty(); i++) {
        if (s.q.front().kind == Op::WAIT) force_event(s.q.front().ev, s.q.front().gen);
        if (!runnable(s)) break; /* only after a reported deadlock */
        run_head(s);
    }
    M.depth--;
}
void force_event(Event *e, uint64_t gen)
{
    if (e->is_done(gen)) return;
    for (Stream *s : M.streams)
        for (size_t i = 0; i < s->q.size(); i++)
            /* the record the wait was made for, not a later one: an event the caller records on several streams may have a later
             * record queued on the very stream that waits */
            if (s->q[i].kind == Op::RECORD && s->q[i].ev == e && s->q[i].gen == gen) {
                force_ops(*s, i + 1);
                return;
            }
    violation("an event wait whose record is on no stream");
    e->mark(gen);
}
void run_all_runnable()
{
    for (bool again = true; again;) {
        again = false;
        for (Stream *s : M.streams)
            while (runnable(*s)) { run_head(*s); again = true; }
    }
}
/* every HIP call passes here once */
void tick()
{
    if (M.c.sched == SCHED_EAGER) run_all_runnable();
    else if (M.c.sched == SCHED_RANDOM && !M.streams.empty())
        for (uint32_t k = rnd() % 4; k > 0; k--) {
            Stream &s = *M.streams[rnd() % M.streams.size()];
            if (runnable(s)) run_head(s);
        }
}
Stream *stream_of(hipStream_t s)
{
    for (Stream *p : M.streams)
        if ((void *)p == (void *)s) return p;
    return nullptr;
}
Event *event_of(hipEvent_t e)
{
    for (Event *p : M.events)
        if ((void *)p == (void *)e) return p;
    return nullptr;
}
void enqueue_work(Stream *s, const std::string &what, std::function<void()> fn)
{
    Op op;
    op.kind = Op::WORK;
    op.fn = std::move(fn);
    op.what = what;
    s->q.push_back(std::move(op));
}
void enqueue_record(Stream *s, Event *e)
{
    Op op;
    op.kind = Op::RECORD;
    op.ev = e;
    op.gen = ++e->recorded;
    e->not_ready_left = (int)(rnd() % 4);
    s->q.push_back(std::move(op));
}

std::string hex(const void *p)
{
    char b[32];
    std::snprintf(b, sizeof b, "%p", p);
    return b;
}

/* ---- copies ----------------------------------------------------------------------------------------------------------------------- */

struct Copy2D { char *d; size_t dp; const char *s; size_t sp, w, h; hipMemcpyKind kind; };
size_t span(size_t pitch, size_t w, size_t h) { return h ? pitch * (h - 1) + w : 0; }
void do_copy(const Copy2D &c)
{
    for (size_t y = 0; y < c.h; y++) std::memmove(c.d + y * c.dp, c.s + y * c.sp, c.w);
}
hipError_t async_copy(const Copy2D &c, hipStream_t hs, const char *name)
{
    Stream *s = stream_of(hs);
    if (!s) return hipErrorInvalidHandle;
    if (c.kind != hipMemcpyHostToDevice && c.kind != hipMemcpyDeviceToHost) return hipErrorInvalidMemcpyDirection;
    const bool h2d = c.kind == hipMemcpyHostToDevice;
    const void *host = h2d ? (const void *)c.s : (const void *)c.d;
    const size_t host_span = h2d ? span(c.sp, c.w, c.h) : span(c.dp, c.w, c.h);
    const std::string what = std::string(name) + (h2d ? " H2D " : " D2H ") + std::to_string(c.w) + "x" + std::to_string(c.h);
    auto run = [c, what] {
        const bool to_dev = c.kind == hipMemcpyHostToDevice;
        const void *dev = to_dev ? (const void *)c.d : (const void *)c.s;
        if (dev_ok(dev, to_dev ? span(c.dp, c.w, c.h) : span(c.sp, c.w, c.h), what + " device side " + hex(dev))) do_copy(c);
    };
    if (!host_locked(host, host_span)) {
        /* pageable host memory: the runtime drains the stream and copies before it returns */
        M.sync_pageable++;
        force_ops(*s, s->q.size());
        run();
        return hipSuccess;
    }
    enqueue_work(s, what, run);
    return hipSuccess;
}

/* ---- the marker operation ------------------------------------------------------------------------------------------------------------ */

struct Marker {
    DbkArgs a;
    int sb, chroma;
    uint64_t h0; /* the scalar operands, folded when the launch was made */
    size_t map_rows;
    std::string name;
    DbkSlOffs sl = {nullptr, 0, 0, 4, 0u}; /* the per-slice operand of the later generations: n_bytes 0 = none */
    int row_mul = 1;                       /* 2: a plane of Cb / Cr pairs, whose rows hold 2 * plane_w samples */
};
/* every operand array in full, as it is NOW */
bool marker_hash(const Marker &m, uint64_t &h)
{
    const DbkArgs &a = m.a;
    h = m.h0;
    if (!dev_ok(a.vert_bs, (size_t)a.n_vert, m.name + " vert bS") || !dev_ok(a.hor_bs, (size_t)a.n_hor, m.name + " hor bS")) return false;
    h = model_fold(h, a.vert_bs, (size_t)a.n_vert);
    h = model_fold(h, a.hor_bs, (size_t)a.n_hor);
    if (a.qp_map) {
        const size_t n = m.map_rows * (size_t)a.map_stride;
        if (!dev_ok(a.qp_map, n, m.name + " QP map")) return false;
        h = model_fold(h, a.qp_map, n);
    }
    if (m.sl.n_bytes) {
        const int n = m.sl.frame_stride ? (a.n_frames > 0 ? a.n_frames : 1) : 1;
        for (int f = 0; f < n; f++) {
            const int8_t *p = m.sl.offs + (size_t)f * (size_t)m.sl.frame_stride;
            if (!dev_ok(p, m.sl.n_bytes, m.name + " per-slice offsets")) return false;
            h = model_fold(h, p, m.sl.n_bytes);
        }
    }
    return true;
}
void run_marker(const Marker &m)
{
    const DbkArgs &a = m.a;
    uint64_t h;
    if (!marker_hash(m, h)) return;
    const int b0 = a.by_begin, b1 = a.by_count ? a.by_begin + a.by_count : a.nby;
    const long long y0 = b0 <= 0 ? 0 : 8ll * b0 - 4, y1 = 8ll * b1 - 4 > a.plane_h ? a.plane_h : 8ll * b1 - 4;
    if (y1 <= y0) return;
    const size_t rb = (size_t)a.plane_w * (size_t)m.sb * (size_t)m.row_mul;
    const int frames = a.n_frames > 0 ? a.n_frames : 1;
    /* the kernels move words of four samples: bases, pitch and frame stride are multiples of that, whatever the transport */
    const size_t word = 4 * (size_t)m.sb;
    if ((uintptr_t)a.src % word || (uintptr_t)a.dst % word || (size_t)a.pitch % word || (size_t)a.frame_stride % word) {
        violation(m.name + " src " + hex(a.src) + " dst " + hex(a.dst) + " pitch " + std::to_string(a.pitch) + ": not aligned to " + std::to_string(word) +
                  " bytes (four samples)");
        return;
    }
    for (int f = 0; f < frames; f++) {
        const uint8_t *src = a.src + (size_t)f * a.frame_stride + (size_t)y0 * a.pitch;
        uint8_t *dst = a.dst + (size_t)f * a.frame_stride + (size_t)y0 * a.pitch;
        const size_t bytes = span((size_t)a.pitch, rb, (size_t)(y1 - y0));
        if (!dev_ok(src, bytes, m.name + " src " + hex(src)) || !dev_ok(dst, bytes, m.name + " dst " + hex(dst))) return;
        for (long long y = y0; y < y1; y++) {
            const uint8_t *s = a.src + (size_t)f * a.frame_stride + (size_t)y * a.pitch;
            uint8_t *d = a.dst + (size_t)f * a.frame_stride + (size_t)y * a.pitch;
            for (size_t x = 0; x < rb; x++) d[x] = (uint8_t)(s[x] ^ model_m(h, m.chroma, (unsigned)y, (unsigned)x));
        }
    }
    M.writes.push_back({a.dst, a.src, a.plane_h, frames, (unsigned)y0, (unsigned)y1});
}

uint64_t fold_ref(const DbkArgs &a)
{
    uint64_t h = kModelHash0;
    h = model_fold(h, a.tc_tab, 52);
    h = model_fold(h, a.beta_tab, 52);
    h = model_fold_int(h, a.tc);
    h = model_fold_int(h, a.beta);
    h = model_fold_int(h, a.max_v);
    if (a.qp_map) {
        h = model_fold_int(h, a.map_stride);
        h = model_fold_int(h, a.ctu_log2);
    }
    return h;
}
uint64_t fold_h265(const DbkH265Args &p)
{
    uint64_t h = kModelHash0 ^ 0x265;
    h = model_fold_int(h, p.qp);
    h = model_fold_int(h, p.tc_off);
    h = model_fold_int(h, p.beta_off);
    h = model_fold_int(h, p.c_qp_offset);
    h = model_fold_int(h, p.base.max_v);
    if (p.base.qp_map) {
        h = model_fold_int(h, p.base.map_stride);
        h = model_fold_int(h, p.base.ctu_log2);
    }
    return h;
}
size_t map_rows_of(const DbkArgs &a, int luma_rows_per_row)
{
    if (!a.qp_map) return 0;
    const size_t luma_h = (size_t)a.plane_h * (size_t)luma_rows_per_row;
    return (luma_h + ((size_t)1 << a.ctu_log2) - 1) >> a.ctu_log2;
}

/* a launch: [record start] kernel(s) [record stop], on the kernel's stream; the events of dbk_set_next_launch_events are one-shot */
hipError_t launch(hipStream_t hs, const std::string &name, std::function<void()> fn)
{
    hipEvent_t e0 = t_start, e1 = t_stop;
    t_start = t_stop = nullptr;
    const bool fail = fault(FAULT_LAUNCH);
    tick();
    if (fail) return hipErrorLaunchFailure;
    Stream *s = stream_of(hs);
    if (!s) return hipErrorInvalidHandle;
    if (e0) enqueue_record(s, event_of(e0));
    enqueue_work(s, name, std::move(fn));
    if (e1) enqueue_record(s, event_of(e1));
    tick();
    return hipSuccess;
}
Marker ref_marker(const DbkArgs &a, int sb, bool chroma, const char *name)
{
    return {a, sb, chroma ? 1 : 0, fold_ref(a), map_rows_of(a, chroma ? 2 : 1), name};
}
Marker h265_marker(const DbkH265Args &p, int sb, bool chroma, int cf, const char *name)
{
    return {p.base, sb, chroma ? 1 : 0, fold_h265(p), map_rows_of(p.base, chroma && cf == 1 ? 2 : 1), name};
}
Marker later_marker(const DbkH265Args &p, const DbkSlOffs &sl, int sb, bool chroma, int cf, const char *name)
{
    DbkH265Args q = p;
    if (sl.n_bytes) q.tc_off = q.beta_off = 0; /* with the operand the call's own pair is not read (_sl) or is zero (_g4, _sp) */
    Marker m = h265_marker(q, sb, chroma, cf, name);
    m.sl = sl;
    return m;
}
/* the plane of pairs: the odd samples' QP offset is a scalar operand of its own */
Marker sp_marker(const DbkH265Args &p, const DbkSlOffs &sl, int cr_qp_offset, int sb, const char *name)
{
    Marker m = later_marker(p, sl, sb, true, 1, name);
    m.h0 = model_fold_int(m.h0, cr_qp_offset);
    m.row_mul = 2;
    return m;
}

/* ---- the SAO operation: dst = src ^ model_m(hash of the scalar operands and of every operand array as it is when the operation runs) ---- */

struct SaoOp {
    DbkSaoArgs a;
    const DbkSaoCtb *cr; /* the odd samples' grid of a plane of pairs, else NULL */
    bool has_nx;
    DbkSaoNox nx;
    int sb, row_mul;
    std::string name;
};
SaoOp sao_op(const DbkSaoArgs &a, const DbkSaoCtb *cr, const DbkSaoNox *nx, int sb, int row_mul, const char *name)
{
    return {a, cr, nx != nullptr && nx->nox != nullptr, nx ? *nx : DbkSaoNox{nullptr, 0, 0}, sb, row_mul, name};
}
bool sao_hash(const SaoOp &o, uint64_t &h)
{
    const DbkSaoArgs &a = o.a;
    h = model_sao_hash0(a.max_v, a.band_shift, a.ctb_log2);
    const size_t frames = a.n_frames > 0 ? (size_t)a.n_frames : 1;
    const size_t cols = (size_t)((a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2), rows = (size_t)((a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2);
    /* a grid of every frame (one, where the frames share it), bounds per frame from the strides */
    auto grid = [&](const void *base, size_t stride, size_t frame_stride, size_t row, size_t n_rows, const char *what) {
        for (size_t f = 0; f < (frame_stride ? frames : 1); f++) {
            const uint8_t *p = (const uint8_t *)base + f * frame_stride;
            if (!dev_ok(p, span(stride, row, n_rows), o.name + " " + what)) return false;
            h = model_fold_rows(h, p, stride, row, n_rows);
        }
        return true;
    };
    const size_t e = sizeof(DbkSaoCtb);
    if (!grid(a.params, (size_t)a.params_stride * e, (size_t)a.params_frame_stride * e, cols * e, rows, "parameters")) return false;
    if (o.cr && !grid(o.cr, (size_t)a.params_stride * e, (size_t)a.params_frame_stride * e, cols * e, rows, "parameters (Cr)")) return false;
    if (a.keep && !grid(a.keep, (size_t)a.keep_stride, (size_t)a.keep_frame_stride, (size_t)(a.plane_w + 7) / 8, (size_t)(a.plane_h + 7) / 8, "keep map")) return false;
    if (o.has_nx && !grid(o.nx.nox, (size_t)o.nx.stride, (size_t)o.nx.frame_stride, cols, rows, "border bytes")) return false;
    return true;
}
/* every row of every frame, src -> dst: the bytes f(y, x) xor-ed in */
template <class F>
void write_planes(const std::string &name, const uint8_t *src, uint8_t *dst, long long pitch, long long frame_stride, int n_frames, int plane_h, size_t rb,
                  int sb, F f)
{
    const size_t word = 4 * (size_t)sb;
    if ((uintptr_t)src % word || (uintptr_t)dst % word || (size_t)pitch % word || (size_t)frame_stride % word) {
        violation(name + " src " + hex(src) + " dst " + hex(dst) + " pitch " + std::to_string(pitch) + ": not aligned to " + std::to_string(word) + " bytes (four samples)");
        return;
    }
    const int frames = n_frames > 0 ? n_frames : 1;
    const size_t bytes = span((size_t)pitch, rb, (size_t)plane_h);
    for (int fr = 0; fr < frames; fr++) {
        const uint8_t *s = src + (size_t)fr * (size_t)frame_stride;
        uint8_t *d = dst + (size_t)fr * (size_t)frame_stride;
        if (!dev_ok(s, bytes, name + " src " + hex(s)) || !dev_ok(d, bytes, name + " dst " + hex(d))) return;
        for (int y = 0; y < plane_h; y++)
            for (size_t x = 0; x < rb; x++) d[(size_t)y * (size_t)pitch + x] = (uint8_t)(s[(size_t)y * (size_t)pitch + x] ^ f((unsigned)y, (unsigned)x));
    }
}
void run_sao(const SaoOp &o)
{
    uint64_t h;
    if (!sao_hash(o, h)) return;
    const DbkSaoArgs &a = o.a;
    write_planes(o.name, a.src, a.dst, a.pitch, a.frame_stride, a.n_frames, a.plane_h, (size_t)a.plane_w * (size_t)o.sb * (size_t)o.row_mul, o.sb,
                 [h](unsigned y, unsigned x) { return model_m(h, kModelSaoPlane, y, x); });
}
/* deblocking + SAO in one kernel: ONE operation, both hashes, the deblocking operands' src to the SAO operands' dst */
struct Fused { Marker m; SaoOp s; };
void run_fused(const Fused &f)
{
    uint64_t hd, hs;
    if (!marker_hash(f.m, hd) || !sao_hash(f.s, hs)) return;
    const DbkSaoArgs &a = f.s.a;
    const int chroma = f.m.chroma;
    write_planes(f.s.name, f.m.a.src, a.dst, a.pitch, a.frame_stride, a.n_frames, a.plane_h, (size_t)a.plane_w * (size_t)f.s.sb * (size_t)f.s.row_mul, f.s.sb,
                 [hd, hs, chroma](unsigned y, unsigned x) { return (uint8_t)(model_m(hd, chroma, y, x) ^ model_m(hs, kModelSaoPlane, y, x)); });
}
hipError_t launch_fused(hipStream_t s, const char *name, std::vector<Fused> fs)
{
    return launch(s, name, [fs] { for (const Fused &f : fs) run_fused(f); });
}

/* launchers that produce operands: a hash of their inputs over their whole output */
struct Derive { std::vector<std::pair<const void *, size_t>> in; std::vector<std::pair<uint8_t *, size_t>> out; std::string name; };
void run_derive(const Derive &d)
{
    uint64_t h = kModelDeriveHash0;
    for (auto &i : d.in) {
        if (!dev_ok(i.first, i.second, d.name + " input")) return;
        h = model_fold(h, i.first, i.second);
    }
    int k = 0;
    for (auto &o : d.out) {
        if (!dev_ok(o.first, o.second, d.name + " output")) return;
        model_derived(h + 0x1000u * (unsigned)k++, o.first, o.second);
    }
}
size_t nv4(int w, int h) { return (size_t)(w / 8 + 1) * (size_t)(h / 4); }
size_t nh4(int w, int h) { return (size_t)(h / 8 + 1) * (size_t)(w / 4); }

} /* namespace */

/* ---- the test's side ------------------------------------------------------------------------------------------------------------------ */

const char *model_fault_name(int kind)
{
    static const char *n[FAULT_KINDS] = {"none", "launch", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipEventRecord", "hipStreamWaitEvent",
                                         "hipEventQuery", "hipMalloc", "hipHostMalloc", "hipExtMallocWithFlags"};
    return kind >= 0 && kind < FAULT_KINDS ? n[kind] : "?";
}
void model_begin(const ModelCase &c)
{
    M.c = c;
    M.rng = 0x9e3779b97f4a7c15ull ^ ((uint64_t)c.seed << 20);
    std::memset(M.calls, 0, sizeof M.calls);
    M.violations.clear();
    M.writes.clear();
    M.sync_pageable = 0;
    M.blocking = M.frees = 0;
    M.depth = 0;
}
int model_blocking_calls() { return M.blocking; }
int model_device_frees() { return M.frees; }
void model_set_supports(bool supports) { M.c.supports = supports; }
int model_calls(int kind) { return M.calls[kind]; }
const std::vector<std::string> &model_violations() { return M.violations; }
int model_sync_pageable_copies() { return M.sync_pageable; }
size_t model_pending_ops()
{
    size_t n = 0;
    for (Stream *s : M.streams) n += s->q.size();
    return n;
}
void model_drain()
{
    for (Stream *s : M.streams) force_ops(*s, s->q.size());
}
const std::vector<ModelWrite> &model_writes() { return M.writes; }
char model_kind_of(const void *p)
{
    for (const Alloc &a : M.allocs)
        if (a.kind != UNMAPPED && (const char *)p >= a.dev && (const char *)p < a.dev + a.n) return "dfpr"[a.kind];
    return 0;
}

void *model_region_alloc(size_t bytes)
{
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), n = (bytes + pg - 1) / pg * pg;
    const int fd = memfd_create("host_frame_sim", 0);
    if (fd < 0 || ftruncate(fd, (off_t)n) != 0) return nullptr;
    void *a = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0), *b = mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (a == MAP_FAILED || b == MAP_FAILED) return nullptr;
    M.regions.push_back({(char *)a, (char *)b, n, fd});
    return a;
}
void model_region_free(void *p)
{
    for (size_t i = 0; i < M.regions.size(); i++)
        if (M.regions[i].primary == p) {
            munmap(M.regions[i].primary, M.regions[i].n);
            munmap(M.regions[i].alias, M.regions[i].n);
            close(M.regions[i].fd);
            M.regions.erase(M.regions.begin() + (long)i);
            return;
        }
}

/* ---- the HIP runtime -------------------------------------------------------------------------------------------------------------------- */

extern "C" {

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { tick(); return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "success" : "injected or modelled error"; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t at, int)
{
    *v = at == hipDeviceAttributeIsLargeBar ? (M.c.large_bar ? 1 : 0) : 256;
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { M.blocking++; model_drain(); return hipSuccess; }
hipError_t hipDeviceGetPCIBusId(char *buf, int len, int) { if (len > 0) buf[0] = 0; return hipErrorInvalidDevice; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) { std::memset(p, 0, sizeof(*p)); return hipSuccess; }

static hipError_t device_alloc(void **p, size_t bytes, Kind k)
{
    *p = nullptr;
    if (bytes > ((size_t)1 << 30)) return hipErrorOutOfMemory;
    char *m = (char *)malloc(bytes ? bytes : 1);
    if (!m) return hipErrorOutOfMemory;
    M.allocs.push_back({m, m, bytes ? bytes : 1, k});
    *p = m;
    return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t bytes)
{
    const bool fail = fault(FAULT_MALLOC);
    tick();
    if (fail) { *p = nullptr; return hipErrorOutOfMemory; }
    return device_alloc(p, bytes, DEVICE);
}
hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned)
{
    const bool fail = fault(FAULT_EXT_MALLOC);
    tick();
    if (fail) { *p = nullptr; return hipErrorOutOfMemory; }
    if (M.c.push_unmapped) {
        /* an address with no mapping behind it, never written through: msync answers ENOMEM for it */
        char *const nowhere = (char *)(uintptr_t)0x10000000u;
        const long pg = sysconf(_SC_PAGESIZE);
        if (msync(nowhere, (size_t)pg, MS_ASYNC) != 0 && msync(nowhere + ((bytes - 1) & ~(size_t)(pg - 1)), (size_t)pg, MS_ASYNC) != 0) {
            M.allocs.push_back({nowhere, nowhere, bytes, UNMAPPED});
            *p = nowhere;
            return hipSuccess;
        }
    }
    return device_alloc(p, bytes, FINE);
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned)
{
    const bool fail = fault(FAULT_HOST_MALLOC);
    tick();
    if (fail) { *p = nullptr; return hipErrorOutOfMemory; }
    return device_alloc(p, bytes, PINNED);
}
static hipError_t release(void *p, bool host)
{
    if (!p) return hipSuccess;
    model_drain(); /* as the runtime: a free waits for the device */
    for (size_t i = 0; i < M.allocs.size(); i++) {
        const Alloc &a = M.allocs[i];
        if (a.host != p || a.kind == REGISTERED || (a.kind == PINNED) != host) continue;
        if (a.kind != UNMAPPED) free(a.host);
        M.allocs.erase(M.allocs.begin() + (long)i);
        return hipSuccess;
    }
    return hipErrorInvalidValue;
}
hipError_t hipFree(void *p) { if (p) M.frees++; return release(p, false); }
hipError_t hipHostFree(void *p) { return release(p, true); }
hipError_t hipHostRegister(void *p, size_t bytes, unsigned)
{
    tick();
    char *c = (char *)p, *dev = c;
    for (const Region &r : M.regions)
        if (c >= r.primary && c + bytes <= r.primary + r.n) dev = r.alias + (c - r.primary);
    for (const Alloc &a : M.allocs)
        if (a.kind == REGISTERED && c < a.host + a.n && a.host < c + bytes) return hipErrorHostMemoryAlreadyRegistered;
    M.allocs.push_back({c, dev, bytes, REGISTERED});
    return hipSuccess;
}
hipError_t hipHostUnregister(void *p)
{
    model_drain();
    for (size_t i = 0; i < M.allocs.size(); i++)
        if (M.allocs[i].kind == REGISTERED && M.allocs[i].host == p) {
            M.allocs.erase(M.allocs.begin() + (long)i);
            return hipSuccess;
        }
    return hipErrorHostMemoryNotRegistered;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *at, const void *p)
{
    tick();
    const char *c = (const char *)p;
    for (const Alloc &a : M.allocs) {
        if (a.kind == UNMAPPED || c < a.host || c >= a.host + a.n) continue;
        std::memset(at, 0, sizeof(*at));
        at->type = a.kind == PINNED || a.kind == REGISTERED ? hipMemoryTypeHost : hipMemoryTypeDevice;
        at->hostPointer = a.kind == DEVICE ? nullptr : (void *)p;
        at->devicePointer = a.dev + (c - a.host);
        return hipSuccess;
    }
    return hipErrorInvalidValue;
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { tick(); std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { tick(); std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind kind, hipStream_t hs)
{
    const bool fail = fault(FAULT_MEMCPY_ASYNC);
    tick();
    if (fail) return hipErrorUnknown;
    const hipError_t e = async_copy({(char *)d, n, (const char *)s, n, n, 1, kind}, hs, "hipMemcpyAsync");
    tick();
    return e;
}
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind kind, hipStream_t hs)
{
    const bool fail = fault(FAULT_MEMCPY2D_ASYNC);
    tick();
    if (fail) return hipErrorUnknown;
    const hipError_t e = async_copy({(char *)d, dp, (const char *)s, sp, w, h, kind}, hs, "hipMemcpy2DAsync");
    tick();
    return e;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    M.streams.push_back(new Stream);
    *s = (hipStream_t)M.streams.back();
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t hs)
{
    for (size_t i = 0; i < M.streams.size(); i++)
        if ((void *)M.streams[i] == (void *)hs) {
            force_ops(*M.streams[i], M.streams[i]->q.size());
            delete M.streams[i];
            M.streams.erase(M.streams.begin() + (long)i);
            return hipSuccess;
        }
    return hipErrorInvalidHandle;
}
hipError_t hipStreamSynchronize(hipStream_t hs)
{
    M.blocking++;
    tick();
    Stream *s = stream_of(hs);
    if (!s) return hipErrorInvalidHandle;
    force_ops(*s, s->q.size());
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t hs, hipEvent_t he, unsigned)
{
    const bool fail = fault(FAULT_STREAM_WAIT_EVENT);
    tick();
    if (fail) return hipErrorUnknown;
    Stream *s = stream_of(hs);
    Event *e = event_of(he);
    if (!s || !e) return hipErrorInvalidHandle;
    if (e->recorded) { /* an event never recorded is no dependency */
        Op op;
        op.kind = Op::WAIT;
        op.ev = e;
        op.gen = e->recorded;
        s->q.push_back(std::move(op));
    }
    tick();
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e)
{
    M.events.push_back(new Event);
    *e = (hipEvent_t)M.events.back();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return hipEventCreate(e); }
hipError_t hipEventDestroy(hipEvent_t he)
{
    for (size_t i = 0; i < M.events.size(); i++)
        if ((void *)M.events[i] == (void *)he) {
            force_event(M.events[i], M.events[i]->recorded);
            delete M.events[i];
            M.events.erase(M.events.begin() + (long)i);
            return hipSuccess;
        }
    return hipErrorInvalidHandle;
}
hipError_t hipEventRecord(hipEvent_t he, hipStream_t hs)
{
    const bool fail = fault(FAULT_EVENT_RECORD);
    tick();
    if (fail) return hipErrorUnknown;
    Stream *s = stream_of(hs);
    Event *e = event_of(he);
    if (!s || !e) return hipErrorInvalidHandle;
    enqueue_record(s, e);
    tick();
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t he)
{
    M.blocking++;
    tick();
    Event *e = event_of(he);
    if (!e) return hipErrorInvalidHandle;
    force_event(e, e->recorded);
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t he)
{
    const bool fail = fault(FAULT_EVENT_QUERY);
    tick();
    if (fail) return hipErrorUnknown;
    Event *e = event_of(he);
    if (!e) return hipErrorInvalidHandle;
    if (e->completed >= e->recorded) return hipSuccess;
    if (M.c.sched != SCHED_LAZY) return hipErrorNotReady;
    if (e->not_ready_left > 0) { e->not_ready_left--; return hipErrorNotReady; }
    force_event(e, e->recorded); /* this event's dependency chain alone */
    return e->completed >= e->recorded ? hipSuccess : hipErrorNotReady;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    Event *ea = event_of(a), *eb = event_of(b);
    *ms = 0.f;
    if (!ea || !eb || !ea->recorded || !eb->recorded) return hipErrorInvalidHandle;
    return ea->completed >= ea->recorded && eb->completed >= eb->recorded ? hipSuccess : hipErrorNotReady;
}

} /* extern "C" */

/* ---- predicates: a case parameter, as in tests/entry_sim ----------------------------------------------------------------------------------- */

bool dbk_packed_supports(const DbkArgs &, int, bool) { return M.c.supports; }
bool dbk_multi_supports(const DbkArgs *, int, const int *) { return M.c.supports; }
bool dbk_packed_h265_supports(const DbkH265Args &, int, bool) { return M.c.supports; }
bool dbk_deblock_sao_supports(const DbkArgs &, const DbkSaoArgs &, int, bool) { return M.c.supports; }
bool dbk_packed_h265_sp_supports(const DbkH265Args &, int) { return M.c.supports; }
bool dbk_deblock_sao_sp_supports(const DbkH265Args &, const DbkSaoArgs &, int) { return M.c.supports; }
/* the count of the real launcher (sao.hip) */
size_t dbk_sao_rows_x2_entries(const DbkSaoArgs &a)
{
    const long long cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    return (size_t)(cols * rows * (a.params_frame_stride ? a.n_frames : 1));
}

/* ---- launchers ------------------------------------------------------------------------------------------------------------------------------ */

void dbk_set_next_launch_events(hipEvent_t start, hipEvent_t stop) { t_start = start; t_stop = stop; }

hipError_t dbk_launch_generic(const DbkArgs &a, int sb, bool chroma, hipStream_t s)
{
    const Marker m = ref_marker(a, sb, chroma, "generic");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed(const DbkArgs &a, int sb, bool chroma, int, hipStream_t s)
{
    const Marker m = ref_marker(a, sb, chroma, "packed");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_multi(const DbkArgs *a, int n, int sb, hipStream_t s)
{
    std::vector<Marker> ms;
    for (int i = 0; i < n; i++) ms.push_back(ref_marker(a[i], sb, i != 0, "packed_multi"));
    return launch(s, "packed_multi", [ms] { for (const Marker &m : ms) run_marker(m); });
}
hipError_t dbk_launch_h265(const DbkH265Args &h, int sb, bool chroma, hipStream_t s)
{
    const Marker m = h265_marker(h, sb, chroma, 1, "h265");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_h265(const DbkH265Args &h, int sb, bool chroma, hipStream_t s)
{
    const Marker m = h265_marker(h, sb, chroma, 1, "packed_h265");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_h265_cf(const DbkH265Args &h, int sb, int cf, hipStream_t s)
{
    const Marker m = h265_marker(h, sb, true, cf, "h265_cf");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_h265_cf(const DbkH265Args &h, int sb, bool chroma, int cf, hipStream_t s)
{
    const Marker m = h265_marker(h, sb, chroma, cf, "packed_h265_cf");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_h265_bs(const void *flags, const void *mv0, const void *mv1, const void *ref0, const void *ref1, int w, int h, uint8_t *vert,
                              uint8_t *hor, uint8_t *cvert, uint8_t *chor, hipStream_t s)
{
    const size_t U = (size_t)(w / 4) * (size_t)(h / 4);
    Derive d{{{flags, 2 * U}, {mv0, 4 * U}, {mv1, 4 * U}, {ref0, 4 * U}, {ref1, 4 * U}}, {{vert, nv4(w, h)}, {hor, nh4(w, h)}}, "h265_bs"};
    if (cvert) {
        d.out.push_back({cvert, nv4(w / 2, h / 2)});
        d.out.push_back({chor, nh4(w / 2, h / 2)});
    }
    return launch(s, d.name, [d] { run_derive(d); });
}
hipError_t dbk_launch_h265_chroma_bs_cf(const uint8_t *vert, const uint8_t *hor, int w, int h, int cf, uint8_t *cvert, uint8_t *chor, hipStream_t s)
{
    const int cw = cf == 3 ? w : w / 2, ch = cf == 1 ? h / 2 : h;
    const Derive d{{{vert, nv4(w, h)}, {hor, nh4(w, h)}}, {{cvert, nv4(cw, ch)}, {chor, nh4(cw, ch)}}, "h265_chroma_bs"};
    return launch(s, d.name, [d] { run_derive(d); });
}
hipError_t dbk_launch_h265_chroma_bs(const uint8_t *vert, const uint8_t *hor, int w, int h, uint8_t *cvert, uint8_t *chor, hipStream_t s)
{
    return dbk_launch_h265_chroma_bs_cf(vert, hor, w, h, 1, cvert, chor, s);
}

/* ---- the later generations of deblocking: as h265_marker, plus the per-slice operand as it is when the operation runs ---- */

hipError_t dbk_launch_h265_sl(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
{
    const Marker m = later_marker(h, sl, sb, cf != 0, cf ? cf : 1, "h265_sl");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_h265_sl(const DbkH265Args &h, const DbkSlOffs &sl, int sb, bool chroma, int cf, hipStream_t s)
{
    const Marker m = later_marker(h, sl, sb, chroma, cf, "packed_h265_sl");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_h265_g4(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
{
    const Marker m = later_marker(h, sl, sb, true, cf, "h265_g4");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_h265_g4(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
{
    const Marker m = later_marker(h, sl, sb, true, cf, "packed_h265_g4");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int sb, hipStream_t s)
{
    const Marker m = sp_marker(h, sl, cr_qp_offset, sb, "h265_sp");
    return launch(s, m.name, [m] { run_marker(m); });
}
hipError_t dbk_launch_packed_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr_qp_offset, int sb, hipStream_t s)
{
    const Marker m = sp_marker(h, sl, cr_qp_offset, sb, "packed_h265_sp");
    return launch(s, m.name, [m] { run_marker(m); });
}

/* ---- producers of per-CTB operands ---- */

hipError_t dbk_launch_h265_slice_offsets(const uint16_t *slice_idx, int in_stride, const int8_t *table, unsigned n_slices, int ctbs_x, int ctbs_y, int8_t *offs,
                                         int offs_stride, hipStream_t s)
{
    Derive d{{{slice_idx, 2 * span((size_t)in_stride, (size_t)ctbs_x, (size_t)ctbs_y)}}, {{(uint8_t *)offs, 2 * span((size_t)offs_stride, (size_t)ctbs_x, (size_t)ctbs_y)}},
             "h265_slice_offsets"};
    if (n_slices) d.in.push_back({table, 2 * (size_t)n_slices});
    return launch(s, d.name, [d] { run_derive(d); });
}
hipError_t dbk_launch_sao_borders(const uint16_t *slice_idx, const uint8_t *slice_across, const uint16_t *tile_idx, int, int ctbs_x, int ctbs_y, int in_stride,
                                  uint8_t *nox, int nox_stride, hipStream_t s)
{
    const size_t n = span((size_t)in_stride, (size_t)ctbs_x, (size_t)ctbs_y);
    Derive d{{{slice_idx, 2 * n}, {slice_across, n}}, {{nox, span((size_t)nox_stride, (size_t)ctbs_x, (size_t)ctbs_y)}}, "sao_borders"};
    if (tile_idx) d.in.push_back({tile_idx, 2 * n});
    return launch(s, d.name, [d] { run_derive(d); });
}
/* 4:2:2 chroma: the caller's grid of every frame into the context's scratch; the operands are re-pointed as the real launchers do */
hipError_t dbk_launch_sao_rows_x2(DbkSaoArgs &a, DbkSaoCtb *dst, hipStream_t s)
{
    const size_t cols = (size_t)((a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2), rows = (size_t)((a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2);
    const size_t e = sizeof(DbkSaoCtb);
    Derive d{{}, {{(uint8_t *)dst, dbk_sao_rows_x2_entries(a) * e}}, "sao_rows_x2"};
    for (size_t f = 0; f < (a.params_frame_stride ? (size_t)a.n_frames : 1); f++)
        d.in.push_back({a.params + f * (size_t)a.params_frame_stride, span((size_t)a.params_stride * e, cols * e, (rows + 1) / 2)});
    a.params = dst;
    a.params_stride = (int)cols;
    a.params_frame_stride = a.params_frame_stride ? (long long)(rows * cols) : 0;
    return launch(s, d.name, [d] { run_derive(d); });
}
hipError_t dbk_launch_sao_nox_rows_x2(const DbkSaoArgs &a, DbkSaoNox &nx, uint8_t *dst, hipStream_t s)
{
    const size_t cols = (size_t)((a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2), rows = (size_t)((a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2);
    const bool per_frame = nx.frame_stride != 0;
    Derive d{{}, {{dst, cols * rows * (per_frame ? (size_t)a.n_frames : 1)}}, "sao_nox_rows_x2"};
    for (size_t f = 0; f < (per_frame ? (size_t)a.n_frames : 1); f++)
        d.in.push_back({nx.nox + f * (size_t)nx.frame_stride, span((size_t)nx.stride, cols, (rows + 1) / 2)});
    nx.nox = dst;
    nx.stride = (int)cols;
    nx.frame_stride = per_frame ? (long long)(rows * cols) : 0;
    return launch(s, d.name, [d] { run_derive(d); });
}

/* ---- the SAO pass ---- */

hipError_t dbk_launch_sao(const DbkSaoArgs &a, int sb, hipStream_t s, const DbkSaoNox *nx)
{
    const SaoOp o = sao_op(a, nullptr, nx, sb, 1, "sao");
    return launch(s, o.name, [o] { run_sao(o); });
}
hipError_t dbk_launch_sao_g4(const DbkSaoArgs &a, int sb, hipStream_t s, const DbkSaoNox *nx)
{
    const SaoOp o = sao_op(a, nullptr, nx, sb, 1, "sao_g4");
    return launch(s, o.name, [o] { run_sao(o); });
}
hipError_t dbk_launch_sao_sp(const DbkSaoArgs &a, const DbkSaoCtb *params_cr, int sb, hipStream_t s, const DbkSaoNox *nx)
{
    const SaoOp o = sao_op(a, params_cr, nx, sb, 2, "sao_sp");
    return launch(s, o.name, [o] { run_sao(o); });
}

/* ---- deblocking + SAO in one kernel, single-plane and multi-plane (plane 0 luma, the others chroma), every generation ---- */

hipError_t dbk_launch_deblock_sao(const DbkArgs &d, const DbkSaoArgs &a, int sb, bool chroma, hipStream_t s)
{
    return launch_fused(s, "deblock_sao", {{ref_marker(d, sb, chroma, "deblock_sao"), sao_op(a, nullptr, nullptr, sb, 1, "deblock_sao")}});
}
hipError_t dbk_launch_deblock_sao_multi(const DbkArgs *d, const DbkSaoArgs *a, int n, int sb, hipStream_t s)
{
    std::vector<Fused> fs;
    for (int i = 0; i < n; i++) fs.push_back({ref_marker(d[i], sb, i != 0, "deblock_sao_multi"), sao_op(a[i], nullptr, nullptr, sb, 1, "deblock_sao_multi")});
    return launch_fused(s, "deblock_sao_multi", fs);
}
namespace {
hipError_t fused_multi(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSlOffs &sl, int n, int sb, int cf, hipStream_t s, const DbkSaoNox *nx, const char *name)
{
    std::vector<Fused> fs;
    for (int i = 0; i < n; i++) fs.push_back({later_marker(h[i], sl, sb, i != 0, cf, name), sao_op(a[i], nullptr, nx ? &nx[i] : nullptr, sb, 1, name)});
    return launch_fused(s, name, fs);
}
const DbkSlOffs kNoOffsets = {nullptr, 0, 0, 4, 0u};
} /* namespace */
hipError_t dbk_launch_deblock_sao_multi_h265(const DbkH265Args *h, const DbkSaoArgs *a, int n, int sb, hipStream_t s)
{
    return fused_multi(h, a, kNoOffsets, n, sb, 1, s, nullptr, "deblock_sao_multi_h265");
}
hipError_t dbk_launch_deblock_sao_h265_cf(const DbkH265Args &h, const DbkSaoArgs &a, int sb, bool chroma, int cf, hipStream_t s, const DbkSaoNox *nx)
{
    return launch_fused(s, "deblock_sao_h265_cf", {{later_marker(h, kNoOffsets, sb, chroma, cf, "deblock_sao_h265_cf"), sao_op(a, nullptr, nx, sb, 1, "deblock_sao_h265_cf")}});
}
hipError_t dbk_launch_deblock_sao_h265_sl(const DbkH265Args &h, const DbkSaoArgs &a, const DbkSlOffs &sl, int sb, bool chroma, int cf, hipStream_t s,
                                          const DbkSaoNox *nx)
{
    return launch_fused(s, "deblock_sao_h265_sl", {{later_marker(h, sl, sb, chroma, cf, "deblock_sao_h265_sl"), sao_op(a, nullptr, nx, sb, 1, "deblock_sao_h265_sl")}});
}
hipError_t dbk_launch_deblock_sao_h265_g4(const DbkH265Args &h, const DbkSaoArgs &a, const DbkSlOffs &sl, int sb, int cf, hipStream_t s, const DbkSaoNox *nx)
{
    return launch_fused(s, "deblock_sao_h265_g4", {{later_marker(h, sl, sb, true, cf, "deblock_sao_h265_g4"), sao_op(a, nullptr, nx, sb, 1, "deblock_sao_h265_g4")}});
}
hipError_t dbk_launch_deblock_sao_multi_h265_cf(const DbkH265Args *h, const DbkSaoArgs *a, int n, int sb, int cf, hipStream_t s, const DbkSaoNox *nx)
{
    return fused_multi(h, a, kNoOffsets, n, sb, cf, s, nx, "deblock_sao_multi_h265_cf");
}
hipError_t dbk_launch_deblock_sao_multi_h265_sl(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSlOffs &sl, int n, int sb, int cf, hipStream_t s,
                                                const DbkSaoNox *nx)
{
    return fused_multi(h, a, sl, n, sb, cf, s, nx, "deblock_sao_multi_h265_sl");
}
hipError_t dbk_launch_deblock_sao_multi_h265_g4(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSlOffs &sl, int n, int sb, int cf, hipStream_t s,
                                                const DbkSaoNox *nx)
{
    return fused_multi(h, a, sl, n, sb, cf, s, nx, "deblock_sao_multi_h265_g4");
}
hipError_t dbk_launch_deblock_sao_h265_sp(const DbkH265Args &h, const DbkSaoArgs &a, const DbkSaoCtb *params_cr, const DbkSlOffs &sl, int cr_qp_offset, int sb,
                                          hipStream_t s, const DbkSaoNox *nx)
{
    return launch_fused(s, "deblock_sao_h265_sp", {{sp_marker(h, sl, cr_qp_offset, sb, "deblock_sao_h265_sp"), sao_op(a, params_cr, nx, sb, 2, "deblock_sao_h265_sp")}});
}
hipError_t dbk_launch_deblock_sao_h265_nv12(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSaoCtb *params_cr, const DbkSlOffs &sl, int cr_qp_offset, int sb,
                                            hipStream_t s, const DbkSaoNox *nx)
{
    return launch_fused(s, "deblock_sao_h265_nv12",
                        {{later_marker(h[0], sl, sb, false, 1, "deblock_sao_h265_nv12"), sao_op(a[0], nullptr, nx ? &nx[0] : nullptr, sb, 1, "deblock_sao_h265_nv12")},
                         {sp_marker(h[1], sl, cr_qp_offset, sb, "deblock_sao_h265_nv12"), sao_op(a[1], params_cr, nx ? &nx[1] : nullptr, sb, 2, "deblock_sao_h265_nv12")}});
}
