/*
 * hip_model.cpp -- the model of hip_model.h: the 31 HIP symbols the two host sources use, and the kernel launchers and predicates
 * of deblock_kernels.h.  Only the thread inside a host entry makes HIP calls (the staging crew never does), so the model needs no
 * lock of its own.  A launcher enqueues a marker operation; see run_marker() for what it does when it executes.
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
    uint64_t recorded = 0, completed = 0; /* generation of the last record enqueued / executed */
    int not_ready_left = 0;
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

bool runnable(const Stream &s) { return !s.q.empty() && !(s.q.front().kind == Op::WAIT && s.q.front().ev->completed < s.q.front().gen); }
void run_head(Stream &s)
{
    Op op = std::move(s.q.front());
    s.q.pop_front();
    if (op.kind == Op::WORK) op.fn();
    else if (op.kind == Op::RECORD && op.ev->completed < op.gen) op.ev->completed = op.gen;
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
    if (e->completed >= gen) return;
    for (Stream *s : M.streams)
        for (size_t i = 0; i < s->q.size(); i++)
            if (s->q[i].kind == Op::RECORD && s->q[i].ev == e && s->q[i].gen >= gen) {
                force_ops(*s, i + 1);
                return;
            }
    violation("an event wait whose record is on no stream");
    e->completed = gen;
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
};
void run_marker(const Marker &m)
{
    const DbkArgs &a = m.a;
    /* every operand array in full, as it is NOW */
    uint64_t h = m.h0;
    if (!dev_ok(a.vert_bs, (size_t)a.n_vert, m.name + " vert bS") || !dev_ok(a.hor_bs, (size_t)a.n_hor, m.name + " hor bS")) return;
    h = model_fold(h, a.vert_bs, (size_t)a.n_vert);
    h = model_fold(h, a.hor_bs, (size_t)a.n_hor);
    if (a.qp_map) {
        const size_t n = m.map_rows * (size_t)a.map_stride;
        if (!dev_ok(a.qp_map, n, m.name + " QP map")) return;
        h = model_fold(h, a.qp_map, n);
    }
    const int b0 = a.by_begin, b1 = a.by_count ? a.by_begin + a.by_count : a.nby;
    const long long y0 = b0 <= 0 ? 0 : 8ll * b0 - 4, y1 = 8ll * b1 - 4 > a.plane_h ? a.plane_h : 8ll * b1 - 4;
    if (y1 <= y0) return;
    const size_t rb = (size_t)a.plane_w * (size_t)m.sb;
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
hipError_t not_modelled() { violation("a launcher the host-frame operators do not use was called"); return hipErrorNotSupported; }

/* launchers that produce operands: a hash of their inputs over their whole output */
struct Derive { std::vector<std::pair<const void *, size_t>> in; std::vector<std::pair<uint8_t *, size_t>> out; std::string name; };
void run_derive(const Derive &d)
{
    uint64_t h = kModelHash0 ^ 0xb5;
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
    M.depth = 0;
}
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
hipError_t hipDeviceSynchronize(void) { model_drain(); return hipSuccess; }
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
hipError_t hipFree(void *p) { return release(p, false); }
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
size_t dbk_sao_rows_x2_entries(const DbkSaoArgs &) { return 0; }

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

/* what the host-frame operators never launch: the device entries of the same sources are tests/entry_sim's */
hipError_t dbk_launch_h265_sl(const DbkH265Args &, const DbkSlOffs &, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_packed_h265_sl(const DbkH265Args &, const DbkSlOffs &, int, bool, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_h265_g4(const DbkH265Args &, const DbkSlOffs &, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_packed_h265_g4(const DbkH265Args &, const DbkSlOffs &, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_h265_sp(const DbkH265Args &, const DbkSlOffs &, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_packed_h265_sp(const DbkH265Args &, const DbkSlOffs &, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_h265_slice_offsets(const uint16_t *, int, const int8_t *, unsigned, int, int, int8_t *, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_sao(const DbkSaoArgs &, int, hipStream_t, const DbkSaoNox *) { return not_modelled(); }
hipError_t dbk_launch_sao_g4(const DbkSaoArgs &, int, hipStream_t, const DbkSaoNox *) { return not_modelled(); }
hipError_t dbk_launch_sao_sp(const DbkSaoArgs &, const DbkSaoCtb *, int, hipStream_t, const DbkSaoNox *) { return not_modelled(); }
hipError_t dbk_launch_sao_borders(const uint16_t *, const uint8_t *, const uint16_t *, int, int, int, int, uint8_t *, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_sao_rows_x2(DbkSaoArgs &, DbkSaoCtb *, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_sao_nox_rows_x2(const DbkSaoArgs &, DbkSaoNox &, uint8_t *, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao(const DbkArgs &, const DbkSaoArgs &, int, bool, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao_multi(const DbkArgs *, const DbkSaoArgs *, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao_multi_h265(const DbkH265Args *, const DbkSaoArgs *, int, int, hipStream_t) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao_h265_cf(const DbkH265Args &, const DbkSaoArgs &, int, bool, int, hipStream_t, const DbkSaoNox *) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao_h265_sl(const DbkH265Args &, const DbkSaoArgs &, const DbkSlOffs &, int, bool, int, hipStream_t, const DbkSaoNox *)
{
    return not_modelled();
}
hipError_t dbk_launch_deblock_sao_h265_g4(const DbkH265Args &, const DbkSaoArgs &, const DbkSlOffs &, int, int, hipStream_t, const DbkSaoNox *)
{
    return not_modelled();
}
hipError_t dbk_launch_deblock_sao_multi_h265_cf(const DbkH265Args *, const DbkSaoArgs *, int, int, int, hipStream_t, const DbkSaoNox *) { return not_modelled(); }
hipError_t dbk_launch_deblock_sao_multi_h265_sl(const DbkH265Args *, const DbkSaoArgs *, const DbkSlOffs &, int, int, int, hipStream_t, const DbkSaoNox *)
{
    return not_modelled();
}
hipError_t dbk_launch_deblock_sao_multi_h265_g4(const DbkH265Args *, const DbkSaoArgs *, const DbkSlOffs &, int, int, int, hipStream_t, const DbkSaoNox *)
{
    return not_modelled();
}
