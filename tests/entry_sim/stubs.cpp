/*
 * stubs.cpp -- what deblock_host.cpp and deblock_host_h265.cpp leave undefined, for a CPU build of the C-ABI entries: the HIP
 * runtime (one device; hipMalloc is host memory; streams and events are numbered handles) and the kernel translation units'
 * launchers and predicates.  A launcher writes one trace line -- its name and the operands that tell launches apart -- and
 * returns an error on the case's k-th launch; a predicate answers as the case says.  Nothing here touches a GPU.
 */
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <vector>

#include "../../gpu_video_codec_amd/csrc/deblock_kernels.h"
#include "entry_sim.h"

SimCtl g_sim;
#ifdef HEVCDBK_DIAG
DbkDiag g_dbk_diag; /* the diagnostic build's knobs live in the kernel translation unit */
#endif

namespace {

struct Block { char *p; size_t n; int k; };
std::vector<Block> g_blocks;

void line(const std::string &s) { g_sim.trace += s + "\n"; }

std::string handle(const char *kind, const void *h)
{
    if (!h) return std::string(kind) + "0";
    return std::string(kind) + std::to_string((uintptr_t)h & 0xfffu);
}
std::string st(hipStream_t s) { return (uintptr_t)s == 0x7770 ? "caller" : handle("st", s); }
std::string ev(hipEvent_t e) { return handle("ev", e); }

/* k-th launch of the case */
hipError_t launched(const std::string &what)
{
    const bool fail = ++g_sim.n_launch == g_sim.fail_at;
    line(what + (fail ? " -> FAIL" : ""));
    return fail ? hipErrorLaunchFailure : hipSuccess;
}

struct Out {
    std::ostringstream o;
    Out(const char *name) { o << name << ":"; }
    template <class T> Out &operator()(const char *k, const T &v) { o << " " << k << "=" << v; return *this; }
    Out &p(const char *k, const void *v) { o << " " << k << "=" << sim_ptr(v); return *this; }
    hipError_t go() { return launched(o.str()); }
};

void put(Out &o, const DbkArgs &a)
{
    o.p("src", a.src).p("dst", a.dst)("pitch", a.pitch)("fs", a.frame_stride)("w", a.plane_w)("h", a.plane_h)("nbx", a.nbx)("nby", a.nby)
        ("nf", a.n_frames).p("vbs", a.vert_bs).p("hbs", a.hor_bs)("vbss", a.vert_bs_stride)("hbss", a.hor_bs_stride)("nv", a.n_vert)
        ("nh", a.n_hor)("vst", a.vstride)("hst", a.hstride)("lbx", a.limit_bx)("lby", a.limit_by)("tc", a.tc)("beta", a.beta)
        ("max", a.max_v)("shift", a.shift).p("map", a.qp_map)("mst", a.map_stride)("ctu", a.ctu_log2)("mfs", a.map_frame_stride)
        ("tc51", (int)a.tc_tab[51])("beta51", (int)a.beta_tab[51])("ovr", a.map_override)("cus", a.n_cus)("by", a.by_begin)("byn", a.by_count);
}
void put(Out &o, const DbkH265Args &h)
{
    put(o, h.base);
    o("qp", h.qp)("tc_off", h.tc_off)("beta_off", h.beta_off)("cqp", h.c_qp_offset);
}
void put(Out &o, const DbkSaoArgs &a)
{
    o.p("s.src", a.src).p("s.dst", a.dst)("s.pitch", a.pitch)("s.fs", a.frame_stride)("s.w", a.plane_w)("s.h", a.plane_h)("s.nf", a.n_frames)
        ("s.max", a.max_v)("s.band", a.band_shift).p("s.params", a.params)("s.pst", a.params_stride)("s.pfs", a.params_frame_stride)
        ("s.ctb", a.ctb_log2).p("s.keep", a.keep)("s.kst", a.keep_stride)("s.kfs", a.keep_frame_stride);
}
void put(Out &o, const DbkSaoNox *nx)
{
    if (!nx) { o("nx", "none"); return; }
    o.p("nx", nx->nox)("nx.st", nx->stride)("nx.fs", nx->frame_stride);
}
void put(Out &o, const DbkSlOffs &sl)
{
    o.p("sl", sl.offs)("sl.st", sl.stride)("sl.fs", sl.frame_stride)("sl.ctb", sl.ctb_log2)("sl.bytes", sl.n_bytes);
}

/* which of the caller's planes the operands speak of: the predicates' answers are one bit per plane, asked as luma or as chroma */
bool answer(unsigned mask, const void *src, bool chroma = false)
{
    const unsigned long long i = (uintptr_t)src / sim_plane_base(0);
    return (mask >> ((i >= 1 && i <= 3 ? i - 1 : 3) + (chroma ? 4 : 0))) & 1u;
}

} /* namespace */

std::string sim_ptr(const void *p)
{
    if (!p) return "0";
    for (const Block &b : g_blocks)
        if ((const char *)p >= b.p && (const char *)p < b.p + (b.n ? b.n : 1))
            return "dev" + std::to_string(b.k) + "+" + std::to_string((const char *)p - b.p);
    std::ostringstream o;
    o << std::hex << "0x" << (uintptr_t)p;
    return o.str();
}
std::string sim_dev_name(const void *p)
{
    for (const Block &b : g_blocks)
        if (b.p == p) return "dev" + std::to_string(b.k);
    return "-";
}
std::string sim_event_name(const void *e) { return e ? ev((hipEvent_t)e) : "-"; }
void sim_new_case()
{
    for (const Block &b : g_blocks) free(b.p); /* a context that was destroyed has freed its own */
    g_blocks.clear();
    g_sim = SimCtl();
}

/* ---- the HIP runtime ---------------------------------------------------------------------------------------------------------- */

extern "C" {

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { line("hipSetDevice"); return g_sim.set_device_fails ? hipErrorInvalidDevice : hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorLaunchFailure ? "launch failure" : (e == hipSuccess ? "success" : "error"); }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipDeviceGetPCIBusId(char *buf, int len, int) { if (len > 0) buf[0] = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) { std::memset(p, 0, sizeof(*p)); return hipSuccess; }

hipError_t hipMalloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (bytes > ((size_t)1 << 30)) return hipErrorOutOfMemory;
    char *m = (char *)malloc(bytes ? bytes : 1);
    if (!m) return hipErrorOutOfMemory;
    g_blocks.push_back({m, bytes, g_sim.n_dev});
    line("hipMalloc dev" + std::to_string(g_sim.n_dev++) + " bytes=" + std::to_string(bytes));
    *p = m;
    return hipSuccess;
}
hipError_t hipFree(void *p)
{
    for (size_t i = 0; i < g_blocks.size(); i++)
        if (g_blocks[i].p == p) {
            line("hipFree dev" + std::to_string(g_blocks[i].k));
            free(p);
            g_blocks.erase(g_blocks.begin() + (long)i);
            return hipSuccess;
        }
    return p ? hipErrorInvalidValue : hipSuccess;
}
hipError_t hipExtMallocWithFlags(void **p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { *p = malloc(bytes ? bytes : 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipHostRegister(void *, size_t, unsigned) { return hipSuccess; }
hipError_t hipHostUnregister(void *) { return hipSuccess; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *, const void *) { return hipErrorInvalidValue; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { std::memmove(d, s, n); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t)
{
    for (size_t y = 0; y < h; y++) std::memmove((char *)d + y * dp, (const char *)s + y * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) { std::memset(d, v, n); return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)(uintptr_t)(0x5000 + ++g_sim.n_stream); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t s) { line("hipStreamSynchronize " + st(s)); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { line("hipStreamWaitEvent " + st(s) + " " + ev(e)); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)(uintptr_t)(0xe000 + ++g_sim.n_ev); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    *e = (hipEvent_t)(uintptr_t)(0xe000 + ++g_sim.n_ev);
    line("hipEventCreateWithFlags " + ev(*e));
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { line("hipEventRecord " + ev(e) + " " + st(s)); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { line("hipEventSynchronize " + ev(e)); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

} /* extern "C" */

/* ---- the predicates ----------------------------------------------------------------------------------------------------------- */

bool dbk_packed_supports(const DbkArgs &a, int, bool chroma) { return answer(g_sim.packed_mask, a.src, chroma); }
bool dbk_multi_supports(const DbkArgs *, int, const int *) { return false; }
bool dbk_packed_h265_supports(const DbkH265Args &h, int, bool chroma) { return answer(g_sim.packed_mask, h.base.src, chroma); }
bool dbk_deblock_sao_supports(const DbkArgs &d, const DbkSaoArgs &, int, bool chroma) { return answer(g_sim.fused_mask, d.src, chroma); }
bool dbk_packed_h265_sp_supports(const DbkH265Args &h, int) { return answer(g_sim.sp_mask, h.base.src); }

size_t dbk_sao_rows_x2_entries(const DbkSaoArgs &a)
{
    const long long cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    return (size_t)(cols * rows * (a.params_frame_stride ? a.n_frames : 1));
}

/* ---- the launchers ------------------------------------------------------------------------------------------------------------ */

void dbk_set_next_launch_events(hipEvent_t, hipEvent_t) {}

#define LAUNCH(name, body)  \
    {                       \
        Out o(name);        \
        body;               \
        return o.go();      \
    }

hipError_t dbk_launch_generic(const DbkArgs &a, int sb, bool chroma, hipStream_t s) LAUNCH("generic", (put(o, a), o("sb", sb)("chroma", chroma)("s", st(s))))
hipError_t dbk_launch_packed(const DbkArgs &a, int sb, bool chroma, int mode, hipStream_t s)
    LAUNCH("packed", (put(o, a), o("sb", sb)("chroma", chroma)("mode", mode)("s", st(s))))
hipError_t dbk_launch_packed_multi(const DbkArgs *a, int n, int sb, hipStream_t s)
    LAUNCH("packed_multi", ([&] { for (int i = 0; i < n; i++) put(o, a[i]); }(), o("n", n)("sb", sb)("s", st(s))))

hipError_t dbk_launch_h265(const DbkH265Args &h, int sb, bool chroma, hipStream_t s) LAUNCH("h265", (put(o, h), o("sb", sb)("chroma", chroma)("s", st(s))))
hipError_t dbk_launch_packed_h265(const DbkH265Args &h, int sb, bool chroma, hipStream_t s)
    LAUNCH("packed_h265", (put(o, h), o("sb", sb)("chroma", chroma)("s", st(s))))
hipError_t dbk_launch_h265_cf(const DbkH265Args &h, int sb, int cf, hipStream_t s) LAUNCH("h265_cf", (put(o, h), o("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_packed_h265_cf(const DbkH265Args &h, int sb, bool chroma, int cf, hipStream_t s)
    LAUNCH("packed_h265_cf", (put(o, h), o("sb", sb)("chroma", chroma)("cf", cf)("s", st(s))))
hipError_t dbk_launch_h265_sl(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
    LAUNCH("h265_sl", (put(o, h), put(o, sl), o("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_packed_h265_sl(const DbkH265Args &h, const DbkSlOffs &sl, int sb, bool chroma, int cf, hipStream_t s)
    LAUNCH("packed_h265_sl", (put(o, h), put(o, sl), o("sb", sb)("chroma", chroma)("cf", cf)("s", st(s))))
hipError_t dbk_launch_h265_g4(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
    LAUNCH("h265_g4", (put(o, h), put(o, sl), o("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_packed_h265_g4(const DbkH265Args &h, const DbkSlOffs &sl, int sb, int cf, hipStream_t s)
    LAUNCH("packed_h265_g4", (put(o, h), put(o, sl), o("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr, int sb, hipStream_t s)
    LAUNCH("h265_sp", (put(o, h), put(o, sl), o("cr", cr)("sb", sb)("s", st(s))))
hipError_t dbk_launch_packed_h265_sp(const DbkH265Args &h, const DbkSlOffs &sl, int cr, int sb, hipStream_t s)
    LAUNCH("packed_h265_sp", (put(o, h), put(o, sl), o("cr", cr)("sb", sb)("s", st(s))))

hipError_t dbk_launch_h265_bs(const void *flags, const void *mv0, const void *mv1, const void *ref0, const void *ref1, int w, int h, uint8_t *vert,
                              uint8_t *hor, uint8_t *cvert, uint8_t *chor, hipStream_t s)
    LAUNCH("h265_bs", o.p("flags", flags).p("mv0", mv0).p("mv1", mv1).p("ref0", ref0).p("ref1", ref1)("w", w)("h", h).p("vert", vert).p("hor", hor)
                          .p("cvert", cvert).p("chor", chor)("s", st(s)))
hipError_t dbk_launch_h265_chroma_bs(const uint8_t *vert, const uint8_t *hor, int w, int h, uint8_t *cvert, uint8_t *chor, hipStream_t s)
    LAUNCH("h265_chroma_bs", o.p("vert", vert).p("hor", hor)("w", w)("h", h).p("cvert", cvert).p("chor", chor)("s", st(s)))
hipError_t dbk_launch_h265_chroma_bs_cf(const uint8_t *vert, const uint8_t *hor, int w, int h, int cf, uint8_t *cvert, uint8_t *chor, hipStream_t s)
    LAUNCH("h265_chroma_bs_cf", o.p("vert", vert).p("hor", hor)("w", w)("h", h)("cf", cf).p("cvert", cvert).p("chor", chor)("s", st(s)))
hipError_t dbk_launch_h265_slice_offsets(const uint16_t *idx, int in_stride, const int8_t *table, unsigned n_slices, int cx, int cy, int8_t *offs,
                                         int offs_stride, hipStream_t s)
    LAUNCH("h265_slice_offsets", o.p("idx", idx)("in_st", in_stride).p("table", table)("n", n_slices)("cx", cx)("cy", cy).p("offs", offs)
                                     ("offs_st", offs_stride)("s", st(s)))

hipError_t dbk_launch_sao(const DbkSaoArgs &a, int sb, hipStream_t s, const DbkSaoNox *nx) LAUNCH("sao", (put(o, a), put(o, nx), o("sb", sb)("s", st(s))))
hipError_t dbk_launch_sao_g4(const DbkSaoArgs &a, int sb, hipStream_t s, const DbkSaoNox *nx)
    LAUNCH("sao_g4", (put(o, a), put(o, nx), o("sb", sb)("s", st(s))))
hipError_t dbk_launch_sao_sp(const DbkSaoArgs &a, const DbkSaoCtb *cr, int sb, hipStream_t s, const DbkSaoNox *nx)
    LAUNCH("sao_sp", (put(o, a), put(o, nx), o.p("cr", cr)("sb", sb)("s", st(s))))
hipError_t dbk_launch_sao_borders(const uint16_t *slice_idx, const uint8_t *across, const uint16_t *tile_idx, int tiles_across, int cx, int cy,
                                  int in_stride, uint8_t *nox, int nox_stride, hipStream_t s)
    LAUNCH("sao_borders", o.p("slice", slice_idx).p("across", across).p("tile", tile_idx)("tiles_across", tiles_across)("cx", cx)("cy", cy)
                              ("in_st", in_stride).p("nox", nox)("nox_st", nox_stride)("s", st(s)))

/* the two launchers that change their operands change them as the real ones do */
hipError_t dbk_launch_sao_rows_x2(DbkSaoArgs &a, DbkSaoCtb *dst, hipStream_t s)
{
    Out o("sao_rows_x2");
    put(o, a);
    o.p("to", dst)("s", st(s));
    const int cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    a.params = dst;
    a.params_stride = cols;
    a.params_frame_stride = a.params_frame_stride ? (long long)rows * cols : 0;
    return o.go();
}
hipError_t dbk_launch_sao_nox_rows_x2(const DbkSaoArgs &a, DbkSaoNox &nx, uint8_t *dst, hipStream_t s)
{
    Out o("sao_nox_rows_x2");
    put(o, a);
    put(o, &nx);
    o.p("to", dst)("s", st(s));
    const int cols = (a.plane_w + (1 << a.ctb_log2) - 1) >> a.ctb_log2, rows = (a.plane_h + (1 << a.ctb_log2) - 1) >> a.ctb_log2;
    nx.nox = dst;
    nx.stride = cols;
    nx.frame_stride = nx.frame_stride ? (long long)rows * cols : 0;
    return o.go();
}

hipError_t dbk_launch_deblock_sao(const DbkArgs &d, const DbkSaoArgs &a, int sb, bool chroma, hipStream_t s)
    LAUNCH("deblock_sao", (put(o, d), put(o, a), o("sb", sb)("chroma", chroma)("s", st(s))))
hipError_t dbk_launch_deblock_sao_multi(const DbkArgs *d, const DbkSaoArgs *a, int n, int sb, hipStream_t s)
    LAUNCH("deblock_sao_multi", ([&] { for (int i = 0; i < n; i++) { put(o, d[i]); put(o, a[i]); } }(), o("n", n)("sb", sb)("s", st(s))))
hipError_t dbk_launch_deblock_sao_multi_h265(const DbkH265Args *h, const DbkSaoArgs *a, int n, int sb, hipStream_t s)
    LAUNCH("deblock_sao_multi_h265", ([&] { for (int i = 0; i < n; i++) { put(o, h[i]); put(o, a[i]); } }(), o("n", n)("sb", sb)("s", st(s))))
hipError_t dbk_launch_deblock_sao_h265_cf(const DbkH265Args &h, const DbkSaoArgs &a, int sb, bool chroma, int cf, hipStream_t s, const DbkSaoNox *nx)
    LAUNCH("deblock_sao_h265_cf", (put(o, h), put(o, a), put(o, nx), o("sb", sb)("chroma", chroma)("cf", cf)("s", st(s))))
hipError_t dbk_launch_deblock_sao_h265_sl(const DbkH265Args &h, const DbkSaoArgs &a, const DbkSlOffs &sl, int sb, bool chroma, int cf, hipStream_t s,
                                          const DbkSaoNox *nx)
    LAUNCH("deblock_sao_h265_sl", (put(o, h), put(o, a), put(o, sl), put(o, nx), o("sb", sb)("chroma", chroma)("cf", cf)("s", st(s))))
hipError_t dbk_launch_deblock_sao_h265_g4(const DbkH265Args &h, const DbkSaoArgs &a, const DbkSlOffs &sl, int sb, int cf, hipStream_t s,
                                          const DbkSaoNox *nx)
    LAUNCH("deblock_sao_h265_g4", (put(o, h), put(o, a), put(o, sl), put(o, nx), o("sb", sb)("cf", cf)("s", st(s))))

namespace {
void put_multi(Out &o, const DbkH265Args *h, const DbkSaoArgs *a, const DbkSaoNox *nx, int n)
{
    for (int i = 0; i < n; i++) {
        put(o, h[i]);
        put(o, a[i]);
        put(o, nx ? &nx[i] : nullptr);
    }
}
} /* namespace */
hipError_t dbk_launch_deblock_sao_multi_h265_cf(const DbkH265Args *h, const DbkSaoArgs *a, int n, int sb, int cf, hipStream_t s, const DbkSaoNox *nx)
    LAUNCH("deblock_sao_multi_h265_cf", (put_multi(o, h, a, nx, n), o("n", n)("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_deblock_sao_multi_h265_sl(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSlOffs &sl, int n, int sb, int cf, hipStream_t s,
                                                const DbkSaoNox *nx)
    LAUNCH("deblock_sao_multi_h265_sl", (put_multi(o, h, a, nx, n), put(o, sl), o("n", n)("sb", sb)("cf", cf)("s", st(s))))
hipError_t dbk_launch_deblock_sao_multi_h265_g4(const DbkH265Args *h, const DbkSaoArgs *a, const DbkSlOffs &sl, int n, int sb, int cf, hipStream_t s,
                                                const DbkSaoNox *nx)
    LAUNCH("deblock_sao_multi_h265_g4", (put_multi(o, h, a, nx, n), put(o, sl), o("n", n)("sb", sb)("cf", cf)("s", st(s))))
