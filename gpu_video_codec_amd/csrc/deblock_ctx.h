/*
 * deblock_ctx.h -- PRIVATE to the library: the context behind `hevcdbk_context *` and the host-side helpers the C-ABI
 * translation units share (deblock_host.cpp: context, plumbing, reference-exact operators, file operators;
 * deblock_host_h265.cpp: spec-exact mode and SAO).  Nothing here is exported (the library is built with hidden visibility).
 * Of the steps the host-frame operators are made of, those the spec-exact frame entry takes too are declared here (FrameLayout,
 * crew_copy_frame, set_timing, GpuDrain); the others and the transports themselves are internal to deblock_host.cpp.
 */
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "../../include/hevc_deblock.h"
#include "deblock_kernels.h"

namespace dbkh { class StageCrew; }

struct Growable {
    void *p = nullptr;
    size_t cap = 0;
};

struct hevcdbk_context {
    int device = 0;
    int n_cus = 0; /* compute units (hipDeviceAttributeMultiprocessorCount): sizes the persistent stripe launches */
    hipStream_t compute = nullptr, h2d = nullptr, d2h = nullptr;
    hipEvent_t ev[16] = {};
    std::string last_error;
    /* staging for the host-frame operator: pinned host + device, grown on demand */
    Growable pin[3], dev[3];
    Growable pin_bs, dev_bs, dev_map, dev_units;
    Growable dev_tmp; /* the deblocked planes between the two launches of hevc_deblock_sao_*_device where the fused kernel does not apply */
    hipEvent_t tmp_ev = nullptr; /* end of the last launch that read dev_tmp: the next user of the scratch plane waits for it */
    bool tmp_used = false;
    Growable dev_sao; /* SAO parameters of 4:2:2 chroma planes rewritten for square CTBs (dbk_launch_sao_rows_x2) */
    hipEvent_t sao_ev = nullptr; /* end of the last launch that read dev_sao */
    bool sao_used = false;
    std::vector<hipEvent_t> timed_events;
    /* streaming operator: ring of kSeqSlots frames in flight */
    static constexpr int kSeqSlots = 3;
    Growable seq_pin[kSeqSlots][3], seq_dev[kSeqSlots][3];
    hipEvent_t seq_ev[kSeqSlots][3] = {}; /* [slot][0 = h2d done, 1 = kernels done, 2 = d2h done] */
    /* dev_bs holds the DEFAULT bS (cpu.h:92-99) of this geometry when bs_default_at == dev_bs.p: no re-upload */
    const void *bs_default_at = nullptr;
    unsigned bs_default_w = 0, bs_default_h = 0;
    bool bs_default_chroma = false;
    /* large pageable frames of the host-frame operator: the staging crew (host_crew.h), created at the first such call */
    dbkh::StageCrew *crew = nullptr;
    Growable dev_push; /* fine-grained HBM the crew writes the caller's rows into through the PCIe BAR (large-BAR devices) */
    int large_bar = -1; /* hipDeviceAttributeIsLargeBar, asked once */
    unsigned host_threads = 0; /* threads copying during a call, the caller included; 0 = default (4) */
    std::vector<hevcdbk_strip_trace> trace; /* the strips of the last large-frame call (hevcdbk_last_frame_trace) */
    /* page-locked host ranges this context made: hevcdbk_host_register'ed ones still registered (released with the context) and
     * hevcdbk_host_malloc_pinned ones not yet freed.  is_pinned_host() answers from them: a plane is page-locked when it lies
     * wholly inside one of these ranges */
    struct HostRange { void *p; size_t bytes; };
    std::vector<HostRange> registered, pinned;
};

namespace dbkh {

bool hip_ok(hevcdbk_context *ctx, hipError_t e, const char *what);
#define HIP_TRY(ctx, call)                                  \
    do {                                                    \
        if (!hip_ok((ctx), (call), #call)) return HEVCDBK_ERR_HIP; \
    } while (0)

int bind(hevcdbk_context *ctx);                                             /* hipSetDevice(ctx->device) */
int grow_pinned(hevcdbk_context *ctx, Growable &g, size_t bytes);
int grow_device(hevcdbk_context *ctx, Growable &g, size_t bytes);
bool bad_depth(unsigned bit_depth, unsigned sample_bytes);
/* true when the `bytes` at p lie in ONE page-locked range this context made (hevcdbk_host_register, hevcdbk_host_malloc_pinned),
 * which the GPU can DMA from directly; *dev_ptr (if asked for) = the address a KERNEL uses for p */
bool is_pinned_host(const hevcdbk_context *ctx, const void *p, size_t bytes, void **dev_ptr = nullptr);
/* the bytes a plane of h rows spans: pitch * (h - 1) + row_bytes */
inline size_t plane_span(size_t pitch, size_t row_bytes, unsigned h) { return h ? pitch * (h - 1) + row_bytes : 0; }

/* Every path out of a host-frame operator that is not HEVCDBK_OK waits for the GPU: kernels and DMAs of earlier strips or frames may
 * still be storing into the ring, the push buffer or the caller's own page-locked planes, and the header promises that transfers
 * have completed when the operators return.  It lives in the entry and the crew's guard (CrewJobs) in the transport function the entry
 * calls, so it runs after the crew has been waited for, and before the caller gets its planes back.  Errors are ignored here: the call
 * is failing already. */
struct GpuDrain {
    hevcdbk_context *ctx;
    bool ok = false; /* set on the way out of a call that succeeded: it has waited for its own work */
    ~GpuDrain()
    {
        if (ok) return;
        (void)hipStreamSynchronize(ctx->h2d);
        (void)hipStreamSynchronize(ctx->compute);
        (void)hipStreamSynchronize(ctx->d2h);
        (void)hipGetLastError();
    }
};
int check_frame(const hevcdbk_frame &f, bool &chroma);
int check_bs(const hevcdbk_bs *bs, unsigned W, unsigned H, bool chroma);
int planes_to_args(const hevcdbk_device_planes *p, unsigned qp, const hevcdbk_tables *tables, DbkArgs &a);
int launch(hevcdbk_context *ctx, const DbkArgs &a0, int sample_bytes, bool chroma, int variant, hipStream_t s);
/* host side of the frame operators (deblock_host.cpp): the staging crew, and HBM the crew writes through the PCIe BAR */
int ensure_crew(hevcdbk_context *ctx);
/* fine-grained device memory of at least `bytes` that the host's cores can write (large-BAR devices), or NULL: no such memory here */
uint8_t *push_buffer(hevcdbk_context *ctx, size_t bytes);
/* a frame in staging (the reference allocates per call, gpu.cu:1103-1169 + 1236-1244; here it persists): tight rows, the planes one
 * after the other, each at a multiple of `align` bytes (256: ONE pinned and ONE device buffer, so a small frame moves in one DMA) */
struct FrameLayout {
    int npl; unsigned pw[3], ph[3], sb;
    size_t row_bytes[3], plane_bytes[3], plane_off[3], frame_bytes; /* 0 for the planes a frame does not have */
};
FrameLayout frame_layout(int npl, const unsigned *pw, const unsigned *ph, unsigned sb, size_t align = 256);
/* every plane of `frame` (tight rows at base + L.plane_off[i]) copied by the crew and the calling thread, which returns when all of
 * it is done.  to_frame: base -> the caller's planes, else the caller's planes -> base; base_is_device: base is HBM seen through the
 * BAR (streaming stores, flushed by a read) */
int crew_copy_frame(hevcdbk_context *ctx, const hevcdbk_frame *frame, const FrameLayout &L, uint8_t *base, bool to_frame, bool base_is_device);
/* the reference's figures of one frame (sums of its serial phases, gpu.cu:1292-1303) and the wall clock of the call; t may be NULL */
inline void set_timing(hevcdbk_timing *t, double exec_s, double copy_s, double wall_s)
{
    if (!t) return;
    t->exec_s = exec_s; t->copy_s = copy_s; t->total_s = exec_s + copy_s; /* gpu.cu:1302 */
    t->pipelined_s = wall_s;
}

} /* namespace dbkh */
