/*
 * hevc_deblock.h -- C ABI of the MI355X-native HEVC in-loop deblocking filter.
 *
 * This is the drop-in boundary for the one hot path of RomanKazantsev/gpu_video_codec:
 * the per-frame deblocking filter that main.cu drives through ExecuteCpu / ExecuteGpu.
 * Every entry point below names the reference interface it replaces.  Citations:
 *   cpu.h  = hevc_deblocking_filter/hevc_deblocking_filter_cpu.h
 *   gpu.cu = hevc_deblocking_filter/hevc_deblocking_filter_gpu.cu
 *   main.cu = hevc_deblocking_filter/main.cu
 *
 * The implementation behind this header is hand-written HIP for gfx950 only.  There is no
 * CPU fallback: every compute entry point returns HEVCDBK_ERR_HIP when no HIP device is usable.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Results are bit-exact with the
 * reference's single-thread CPU path (cpu.h:134-993) including its quirks (SURVEY.md 8a Q-list):
 * frames are UN-padded W x H planes here, the reference's 4-sample zero padding (cpu.h:55-71)
 * is implicit.
 */
#ifndef HEVC_DEBLOCK_H
#define HEVC_DEBLOCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the library is built with hidden visibility: only the entry points below leave it */
#if defined(__GNUC__) || defined(__clang__)
#define HEVCDBK_API __attribute__((visibility("default")))
#else
#define HEVCDBK_API
#endif

/* ---- error codes: the reference throws `const char *` at three sites; the ABI returns ---- */
#define HEVCDBK_OK               0
#define HEVCDBK_ERR_FILE_SIZE   (-1) /* cpu.h:43-45  / gpu.cu:1082-1084 "Incorrect file size" */
#define HEVCDBK_ERR_DIMENSIONS  (-2) /* cpu.h:46-48  / gpu.cu:1085-1087 "Width and height of image must be multiplier of sample block size" */
#define HEVCDBK_ERR_BS_SIZE     (-3) /* cpu.h:122-123 "Incorrect size of input boundary strenght array" */
#define HEVCDBK_ERR_HIP         (-4) /* a HIP call failed or no device (reference prints and continues, gpu.cu:1271-1288) */
#define HEVCDBK_ERR_ARG         (-5)
#define HEVCDBK_ERR_NOMEM       (-6)
#define HEVCDBK_ERR_IO          (-7)
#define HEVCDBK_ERR_UNSUPPORTED (-8) /* alignment / bit depth outside what the kernels handle */

HEVCDBK_API const char *hevcdbk_strerror(int code);

/* ---- context: replaces the file-scope globals of gpu.cu:37-77 (one per device, re-entrant) ---- */
typedef struct hevcdbk_context hevcdbk_context;

HEVCDBK_API int hevcdbk_device_count(void);
/* binds to HIP device `device`, creates the compute stream and the two copy side streams */
HEVCDBK_API int hevcdbk_create(int device, hevcdbk_context **ctx);
HEVCDBK_API void hevcdbk_destroy(hevcdbk_context *ctx);
/* text of the last HIP failure seen by this context ("" if none) */
HEVCDBK_API const char *hevcdbk_last_error(const hevcdbk_context *ctx);
/* GetGpuDeviceInfo() equivalent (main.cu:92-107): fills name, CU count, memory */
typedef struct {
    char name[256];
    char gcn_arch[64];
    int compute_units;
    int wavefront_size;
    int max_threads_per_block;
    size_t total_global_mem;
    size_t shared_mem_per_block;
    size_t total_const_mem;
} hevcdbk_device_info;
HEVCDBK_API int hevcdbk_get_device_info(const hevcdbk_context *ctx, hevcdbk_device_info *info);

/* ---- tables and bS helpers ---- */
/* cpu.h:1021-1033 (copies at gpu.cu:80-85, 92-97) */
HEVCDBK_API const unsigned *hevcdbk_default_tc_table(void);   /* 52 entries */
HEVCDBK_API const unsigned *hevcdbk_default_beta_table(void); /* 52 entries */
/* cpu.h:86-87 / 104-105: element counts of the bS arrays of a plane_w x plane_h plane */
HEVCDBK_API size_t hevcdbk_num_vert_bs(unsigned plane_w, unsigned plane_h);
HEVCDBK_API size_t hevcdbk_num_hor_bs(unsigned plane_w, unsigned plane_h);
/* cpu.h:92-99 / 110-117 (gpu.cu:1136-1180): the default "all intra" pattern, quirks included */
HEVCDBK_API int hevcdbk_default_bs(unsigned plane_w, unsigned plane_h, uint8_t *vert_bs, uint8_t *hor_bs);

/* ---- operands of hevc_deblocking_filter(frame, bS, QP, tc/beta tables) ---- */

/* frame: replaces ReadYuvFrame's planes (cpu.h:1041-1048) / the pinned planes of gpu.cu:37-45.
 * Un-padded planar 4:2:0; U/V may be NULL for a luma-only call.  Caller owns the memory. */
typedef struct {
    unsigned width, height; /* luma samples, multiples of 8 (cpu.h:46-48); with chroma: multiples of 16 */
    unsigned bit_depth;     /* 8..16; the reference is 8 (cpu.h:1202) */
    unsigned sample_bytes;  /* 1 (bit_depth 8 only) or 2 (little-endian containers) */
    void *plane[3];         /* Y, U, V */
    size_t pitch[3];        /* bytes between rows */
} hevcdbk_frame;

/* bS: replaces SetBoundaryStrenght(vert, n, hor, n) (cpu.h:120-132).  Layouts are the reference's:
 * vert[r*(W/8+1)+bx] = vertical edge at x = 8*bx of block row r; hor[by*(W/8)+c] = horizontal edge
 * at y = 8*by of block column c.  NULL pointers => reference default pattern (cpu.h:92-99).
 * The reference can only override luma; chroma overrides are an extension. */
typedef struct {
    const uint8_t *vert; size_t n_vert;
    const uint8_t *hor;  size_t n_hor;
    const uint8_t *chroma_vert; size_t n_chroma_vert;
    const uint8_t *chroma_hor;  size_t n_chroma_hor;
} hevcdbk_bs;

/* QP: replaces the ctor's Qp (cpu.h:35-37, main.cu:117,125,133).  map != NULL selects the per-CTU
 * map extension (BASELINE config 3b): QP of a 4-line edge segment = (QpP + QpQ + 1) >> 1 of the
 * CTUs holding P0 / Q0 of its first line. */
typedef struct {
    unsigned qp;
    const uint8_t *map;  /* map[cy*map_stride + cx], may be NULL */
    unsigned map_stride;
    unsigned ctu_log2;   /* CTU size in luma samples, log2 (6 => 64) */
} hevcdbk_qp;

/* tc / beta tables: replace beta_table / tc_table (cpu.h:1021-1033).  NULL => the reference's. */
typedef struct {
    const unsigned *tc;   /* 52 entries, each <= 255 */
    const unsigned *beta; /* 52 entries, each <= 255 */
} hevcdbk_tables;

/* the reference's three console figures (gpu.cu:1292, 1302-1303), seconds */
typedef struct {
    double exec_s;  /* "Execution Time without copy on GPU"  : kernels + sync   (gpu.cu:1266-1291) */
    double total_s; /* "Execution Time with copy on GPU"     : exec + copy      (gpu.cu:1302)      */
    double copy_s;  /* "Copy Operation Time with GPU buffers": H2D + D2H        (gpu.cu:1246-1258, 1294-1300) */
    double pipelined_s; /* wall time of the overlapped pinned/async pipeline actually run */
    /* Small frames (<= 2 MiB) are not copied at all: the kernel reads and writes page-locked host memory across PCIe
     * itself, so copy_s is 0 and exec_s contains the PCIe traffic.  Large frames: sums over the strips of the frame. */
} hevcdbk_timing;

/*
 * THE operator.  Replaces ReadYuvFrame::DeblockingFilter (cpu.h:134) and the body of ExecuteGpu
 * (gpu.cu:1246-1300: 7 H2D copies, 3 kernel launches, sync, 3 D2H copies) for a frame in HOST
 * memory, in place.  Frames up to 2 MiB: the fused Y+U+V kernel works on page-locked memory across the
 * link itself.  Larger frames are cut into strips of whole block rows: on a large-BAR device the
 * context's crew of host threads writes the strips into HBM through the BAR while the kernels of
 * earlier strips store their results into page-locked memory (the caller's own planes where those
 * are page-locked / registered with tight rows); elsewhere: pinned staging + hipMemcpyAsync on side
 * streams.  See hevcdbk_set_host_threads / hevcdbk_host_register below.  bs / tables / timing may be NULL.
 */
HEVCDBK_API int hevc_deblocking_filter(hevcdbk_context *ctx, hevcdbk_frame *frame, const hevcdbk_bs *bs,
                           const hevcdbk_qp *qp, const hevcdbk_tables *tables,
                           hevcdbk_timing *timing);

/*
 * Host side of hevc_deblocking_filter on a LARGE frame (> 2 MiB) in ordinary pageable memory -- the frame main.cu:112-133
 * gets from ReadYuvFrame, where the reference copies row by row into cudaMallocHost planes on one thread, outside its
 * timers (gpu.cu:1092-1133).  The frame is cut into strips of whole block rows (the first ones short, so the first DMA
 * starts early); a crew of host threads copies strips into the page-locked ring while earlier strips are on the link, in
 * the kernel or on their way back, and copies finished strips out.
 *   hevcdbk_set_host_threads: how many threads copy during a call, the calling thread included (1 = the caller alone;
 *   0 = the default, 4).  Crew threads are created at the first large pageable frame, run on the CPUs next to the GPU's
 *   host bridge (sysfs local_cpulist) where the process is allowed to, sleep between calls and end with the context.
 */
HEVCDBK_API int hevcdbk_set_host_threads(hevcdbk_context *ctx, unsigned n_threads);
HEVCDBK_API unsigned hevcdbk_get_host_threads(const hevcdbk_context *ctx);

/*
 * For callers that hand the same buffers in again and again (a decoder's picture pool): page-locks [ptr, ptr+bytes) in
 * place (hipHostRegister; the reference's equivalent is allocating the planes with cudaMallocHost, gpu.cu:1092-1099).
 * Planes that lie WHOLLY inside a registered range are worked on or DMA'd where they lie, with no staging copy, by
 * hevc_deblocking_filter and hevc_deblocking_filter_sequence; a plane that begins in a range and runs past its end is staged
 * like pageable memory.  The spec-exact host entries (hevc_deblocking_filter_h265, hevcdbk_h265_filter_frame_cf) always copy
 * the frame through the page-locked ring or the BAR, registered or not.  Memory page-locked by other means (hipHostMalloc or
 * hipHostRegister called by the application, another context) is staged like pageable memory as well: of such memory the runtime
 * tells the kind of a byte, not where its allocation ends.  Transfers of the host-frame operators have completed
 * when they return, with an error code too.  The caller unregisters before freeing the memory.
 */
HEVCDBK_API int hevcdbk_host_register(hevcdbk_context *ctx, void *ptr, size_t bytes);
HEVCDBK_API int hevcdbk_host_unregister(hevcdbk_context *ctx, void *ptr);

/*
 * Where the time of the LAST hevc_deblocking_filter call on a large frame went, strip by strip (measurement aid; the
 * reference prints three sums, gpu.cu:1292-1303).  Host-clock fields are seconds since the call began; a field that does
 * not apply (no staging for page-locked planes; GPU durations when the call had timing == NULL) is 0.
 */
typedef struct {
    int plane;                 /* 0 Y, 1 U, 2 V */
    unsigned row_begin, row_end;
    size_t bytes;
    double stage_begin_s, stage_end_s;     /* the crew's copy into the page-locked ring: first job began / last job ended */
    double enqueue_begin_s, enqueue_end_s; /* H2D + kernel + D2H of the strip handed to the HIP runtime */
    double d2h_seen_s;                     /* the calling thread saw the strip's download complete */
    double unstage_begin_s, unstage_end_s; /* the crew's copy back into the caller's plane */
    double h2d_ms, kernel_ms, d2h_ms;      /* GPU clock, between events on the three streams */
} hevcdbk_strip_trace;
/* copies min(cap, strips) entries to out (may be NULL with cap 0) and stores the strip count in *n_strips */
HEVCDBK_API int hevcdbk_last_frame_trace(const hevcdbk_context *ctx, hevcdbk_strip_trace *out, unsigned cap, unsigned *n_strips);

/*
 * Streaming form for a SEQUENCE of host frames of one geometry (the multi-frame case the reference does
 * not have).  Three frames are in flight: H2D of frame n+1, the kernels of frame n and
 * D2H of frame n-1 overlap on the context's three streams.  Planes that already are page-locked
 * through THIS context (hevcdbk_host_malloc_pinned, hevcdbk_host_register) are DMA'd in place with no staging copy;
 * pageable planes go through the context's pinned ring.  bs / tables are shared by all frames;
 * timing->pipelined_s is the wall time of the whole sequence.  A per-CTU QP map is not accepted here.  Sequences of small
 * 8-bit 4:2:0 frames (<= 2 MiB per frame, at least 4 of them) travel in groups of up to 64 frames instead: packed back to
 * back into one pinned chunk, one DMA each way and one batched launch per group.
 */
HEVCDBK_API int hevc_deblocking_filter_sequence(hevcdbk_context *ctx, hevcdbk_frame *frames, unsigned n_frames,
                                    const hevcdbk_bs *bs, const hevcdbk_qp *qp, const hevcdbk_tables *tables,
                                    hevcdbk_timing *timing);

/*
 * Device-resident form of the same operator, for callers whose planes already live in HBM
 * (the decoder pipeline case, and what bench.py times).  One launch filters n_frames planes of
 * identical geometry.  src and dst are DEVICE pointers and may be equal (in place); blocks are
 * mutually independent so in-place is race-free.
 */
typedef struct {
    const void *src;       /* frame f plane at src + f*frame_stride */
    void *dst;
    size_t pitch;          /* bytes, multiple of 4 */
    size_t frame_stride;   /* bytes */
    unsigned n_frames;
    unsigned plane_w, plane_h; /* samples of THIS plane (chroma: W/2 x H/2) */
    unsigned bit_depth, sample_bytes;
    int is_chroma;         /* chroma block procedure: bS == 2 only, p0/q0 only (cpu.h:450-992) */
    const uint8_t *vert_bs; /* DEVICE; frame f at vert_bs + f*vert_bs_stride (stride 0 = shared) */
    const uint8_t *hor_bs;
    size_t vert_bs_stride, hor_bs_stride;
    const uint8_t *qp_map; /* DEVICE or NULL; frame f at qp_map + f*qp_map_frame_stride */
    unsigned qp_map_stride, ctu_log2; /* entries per map row (< 2^24, HEVCDBK_ERR_UNSUPPORTED otherwise); log2 of the map unit in luma samples, 3 .. 8 (HEVCDBK_ERR_ARG otherwise) */
    size_t qp_map_frame_stride;
} hevcdbk_device_planes;

/* kernel variant selector for hevc_deblocking_filter_device */
#define HEVCDBK_KERNEL_AUTO    0 /* fastest kernel that supports the operands */
#define HEVCDBK_KERNEL_GENERIC 1 /* one lane per offset block, 32-bit scalar arithmetic (all operand kinds) */
#define HEVCDBK_KERNEL_PACKED  2 /* packed 16-bit arithmetic kernel (8-bit samples, scalar QP) */
/* optional, OR-ed into the selector: how the packed kernels deal offset blocks to lanes.  Both maps produce the same
 * bytes; AUTO picks per geometry from measurements. */
#define HEVCDBK_MAP_AUTO   0x000
#define HEVCDBK_MAP_ROWS   0x100 /* one workgroup per block row */
#define HEVCDBK_MAP_LINEAR 0x200 /* row-major block numbering, workgroups renumbered per XCD */
#define HEVCDBK_MAP_MASK   0x700

HEVCDBK_API int hevc_deblocking_filter_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes,
                                  unsigned qp, const hevcdbk_tables *tables, int kernel_variant,
                                  void *hip_stream /* NULL => the context's compute stream */);

/* The planes of a batch of frames in ONE call -- normally Y, U, V of a 4:2:0 batch (planes[0] luma; 1 <= n_planes <= 3; all
 * with the same n_frames).  Replaces the reference's three launches per frame (gpu.cu:1266-1285): when the planes share one
 * sample format that the packed kernels take (8 bit -- the reference's case -- or 16-bit containers up to 12 bit) and a scalar
 * QP they go out as ONE fused launch, whatever the frame size; other operands (a QP map, deeper samples) are launched plane by
 * plane, exactly as n_planes calls of hevc_deblocking_filter_device would.  Same bytes either way. */
HEVCDBK_API int hevc_deblocking_filter_device_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *planes,
                                         unsigned n_planes, unsigned qp, const hevcdbk_tables *tables,
                                         int kernel_variant, void *hip_stream);

/* ---- device memory / stream plumbing for hosts without a HIP binding (ctypes, cgo, JNI) ---- */
HEVCDBK_API int hevcdbk_device_malloc(hevcdbk_context *ctx, size_t bytes, void **dptr);
HEVCDBK_API int hevcdbk_device_free(hevcdbk_context *ctx, void *dptr);
HEVCDBK_API int hevcdbk_host_malloc_pinned(hevcdbk_context *ctx, size_t bytes, void **hptr); /* hipHostMalloc, replaces cudaMallocHost gpu.cu:1103-1169 */
HEVCDBK_API int hevcdbk_host_free_pinned(hevcdbk_context *ctx, void *hptr);
HEVCDBK_API int hevcdbk_memcpy_h2d(hevcdbk_context *ctx, void *dptr, const void *hptr, size_t bytes); /* synchronous */
HEVCDBK_API int hevcdbk_memcpy_d2h(hevcdbk_context *ctx, void *hptr, const void *dptr, size_t bytes);
HEVCDBK_API int hevcdbk_memcpy_d2d(hevcdbk_context *ctx, void *dst, const void *src, size_t bytes);
HEVCDBK_API int hevcdbk_memset_d(hevcdbk_context *ctx, void *dptr, int value, size_t bytes);
HEVCDBK_API int hevcdbk_synchronize(hevcdbk_context *ctx); /* all three streams */
HEVCDBK_API void *hevcdbk_compute_stream(hevcdbk_context *ctx); /* hipStream_t */

/*
 * A destination pool chosen among several allocations.  Where the driver puts a buffer's physical pages decides how fast the
 * kernels for 16-bit containers write into it: identical launches run up to 13 % apart from one allocation to the next, the
 * difference follows the DESTINATION buffer, stays with it for its lifetime, and nothing cheaper than the filter itself
 * predicts it (a fill or a DMA copy does not; it is not address translation: profiles/r04/placement.md).  For a pool that lives
 * long -- a decoder's output pictures -- it pays to look once: `probe` describes a launch exactly as
 * hevc_deblocking_filter_device takes it (its dst field is ignored); the function allocates `candidates` (1 .. 16) buffers of the
 * size that launch writes (frame_stride * (n_frames - 1) + pitch * plane_h), runs the launch into each (one warm-up, three
 * timed), keeps the fastest, frees the others and returns it in *dptr (release with hevcdbk_device_free).  best_ms / worst_ms
 * (may be NULL): the fastest and the slowest candidate's kernel time.  The reference allocates its device planes once per run
 * with cudaMalloc (gpu.cu:1110-1133) and has no such choice to make.
 */
HEVCDBK_API int hevcdbk_device_malloc_probed(hevcdbk_context *ctx, const hevcdbk_device_planes *probe, unsigned qp,
                                             const hevcdbk_tables *tables, unsigned candidates, void **dptr, float *best_ms,
                                             float *worst_ms);

/* Timed replay for benchmarks: launches the device operator `steps` times back-to-back on the
 * compute stream with a HIP event pair around EACH launch, synchronises once at the end and
 * writes the per-launch kernel durations (milliseconds) to kernel_ms[steps].  (= hevcdbk_device_replay with no
 * settling and no warm-up.)  The timing window is the reference's "execution time without copy": kernels + one
 * synchronisation, nothing else (gpu.cu:1266-1291).  n_planes is 1 .. 3 (the planes of one 4:2:0 batch) and every plane
 * holds the same n_frames -- anything else is HEVCDBK_ERR_ARG, here and in hevcdbk_device_replay; the compute stream is
 * drained before the first launch, so work an earlier asynchronous call left on it is outside the window. */
HEVCDBK_API int hevcdbk_device_run_timed(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                             unsigned qp, const hevcdbk_tables *tables, int kernel_variant,
                             unsigned steps, float *kernel_ms);

/* Steady-state replay: ONE uninterrupted stream of [settle launches][warmup launches][steps timed launches] of the device
 * operator on the compute stream, one synchronisation at the very end (same window semantics as above).  Settling is by
 * time: launches go out until the mean duration of the trailing settle_window launches is within settle_tolerance of the
 * mean of the window before it, for at least settle_min_ms and at most settle_max_ms (settle_max_ms == 0: no settling;
 * settle_min_ms == settle_max_ms: a fixed time).  The host stays ahead of the GPU throughout, so the queue never drains
 * between the phases; the front bracket of the timed window is the host observing the end of the last launch before it. */
typedef struct {
    /* in */
    double settle_min_ms, settle_max_ms;
    double settle_tolerance;   /* relative; 0 => 0.005 */
    unsigned settle_window;    /* launches; 0 => 32 */
    unsigned warmup, steps;
    /* out */
    unsigned settle_launches;  /* launches the settle phase issued */
    int settled;               /* 1: the criterion was met before settle_max_ms */
    double settle_ms;          /* host time the settle phase took to issue */
    double settle_tail_mean_ms;/* mean duration of its last settle_window launches */
    double t_begin, t_end;     /* CLOCK_MONOTONIC seconds: end of the launch before the first timed one as seen by the
                                * host / return of the final synchronisation */
    double wall_ms;            /* (t_end - t_begin) * 1e3: host wall clock of the `steps` timed launches */
    double span_ms;            /* GPU timestamps: begin of the first timed launch -> end of the last one */
} hevcdbk_replay;
HEVCDBK_API int hevcdbk_device_replay(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                          unsigned qp, const hevcdbk_tables *tables, int kernel_variant, hevcdbk_replay *replay,
                          float *kernel_ms /* [replay->steps] */);

/* PCI bus id ("0000:0a:00.0") of the context's device, for hosts that read the card's sysfs files (clock / power telemetry);
 * replaces nothing in the reference (GetGpuDeviceInfo, main.cu:92-107, prints properties only).  len >= 13. */
HEVCDBK_API int hevcdbk_device_pci_bus_id(const hevcdbk_context *ctx, char *buf, size_t len);

/* ---- main.cu-shaped harness entry: replaces ExecuteGpu (main.cu:87-90, gpu.cu:1230-1306) ----
 * file in -> filter Y,U,V on the GPU -> file out, printing the reference's three lines.
 * The four launch-dimension arguments are accepted and ignored.  Returns an error code instead of
 * throwing.  `device` selects the HIP device (the reference always uses device 0, main.cu:93). */
HEVCDBK_API int hevcdbk_execute_gpu(const char *input_file_name, const char *output_file_name,
                        unsigned width, unsigned height, unsigned qp,
                        unsigned dimx1, unsigned dimy1, unsigned dimx2, unsigned dimy2, int device);

/*
 * Multi-frame planar 8-bit 4:2:0 file -> file.  The reference's reader takes exactly one frame per file
 * (cpu.h:40-45, gpu.cu:1077-1084: anything else throws "Incorrect file size"); a sequence is what a caller holds in
 * practice, so this entry accepts any whole number of frames (>= 1) and is byte-identical, frame by frame, to running
 * the reference's ReadYuvFrame -> [SetBoundaryStrenght] -> DeblockingFilter -> Save on each.  File reads, GPU work and
 * file writes overlap, chunk by chunk, through three pinned buffers; a chunk (up to 64 frames / 64 MiB, frames back to
 * back as in the file) moves in ONE DMA each way and its planes are filtered as batches of frames whose frame stride is
 * one file frame -- one fused Y+U+V launch per chunk when the geometry allows.  `bs` / `tables` as for hevc_deblocking_filter (NULL = the
 * reference's defaults).  in == out is refused.  timing->pipelined_s = wall time including file I/O.
 */
HEVCDBK_API int hevcdbk_filter_yuv_file(hevcdbk_context *ctx, const char *input_file_name, const char *output_file_name,
                            unsigned width, unsigned height, unsigned qp, const hevcdbk_bs *bs,
                            const hevcdbk_tables *tables, unsigned *n_frames, hevcdbk_timing *timing);

/*
 * The same operator sharded over several GPUs of one node (frames are independent, so there is no exchange
 * step and no collective).  devices[g] is the HIP device of worker g; chunk c of the file (up to 64 frames) is read,
 * filtered and written back at its own offset by worker c mod n_devices, each worker being one host thread with its own
 * context.  A device may be listed more than once (two workers sharing one GPU).  The output is byte-identical to
 * hevcdbk_filter_yuv_file's.  Error codes as there; the first failing worker's code is returned.
 */
HEVCDBK_API int hevcdbk_filter_yuv_file_multi(const int *devices, unsigned n_devices, const char *input_file_name,
                                  const char *output_file_name, unsigned width, unsigned height, unsigned qp,
                                  const hevcdbk_bs *bs, const hevcdbk_tables *tables, unsigned *n_frames,
                                  hevcdbk_timing *timing);

/* ==================================================================================================================
 * Spec-exact mode: ITU-T H.265 (HEVC) clause 8.7.2.
 *
 * The reference's filter is HEVC-shaped but not conformant: it hard-codes bS = 2 (cpu.h:91-99) and one QP per frame
 * (cpu.h:136-137), and its arithmetic differs from the standard in the strong-filter thresholds (cpu.h:1099-1110), the
 * clip of the normal filter's delta (cpu.h:1256), the chroma formula (cpu.h:1453-1458), the hor2 column pairing
 * (cpu.h:383-414) and the filtered frame edges.  The entries below are what a decoder needs instead.  They never change
 * the results of the reference-exact entries above.  Parity: checked against oracle/h265_oracle.c, a restatement of the
 * standard's text written in picture order (no implementation of the standard exists in the reference or in this
 * image: "parity unpinned").
 *
 * bS arrays are 4-sample granular (the standard's unit):
 *   vert: (W/8+1) columns x (H/4) rows, entry (y4, bx) = the edge x = 8*bx over rows 4*y4 .. 4*y4+3
 *   hor:  (H/8+1) rows x (W/4) columns, entry (by, x4) = the edge y = 8*by over columns 4*x4 .. 4*x4+3
 * for a W x H plane; chroma planes carry their own arrays in the chroma plane's geometry (4:2:0 here; the other chroma
 * formats: the _cf entries at the end of this header).  An entry holds the
 * bS in bits 1:0 and two flags: HEVCDBK_H265_KEEP_P / _KEEP_Q leave the P / Q samples unmodified (pcm_loop_filter_
 * disabled_flag with a PCM block, cu_transquant_bypass_flag: nDp / nDq = 0 in 8.7.2.5.7).  Edges on the picture boundary
 * are never filtered, whatever the arrays hold.
 * ================================================================================================================== */
#define HEVCDBK_H265_BS_MASK 3u
#define HEVCDBK_H265_KEEP_P  4u
#define HEVCDBK_H265_KEEP_Q  8u

typedef struct hevcdbk_h265_params {
    int tc_offset_div2;   /* slice_tc_offset_div2 (or pps_tc_offset_div2), -6..6 */
    int beta_offset_div2; /* slice_beta_offset_div2, -6..6 */
    int cb_qp_offset;     /* pps_cb_qp_offset (+ slice_cb_qp_offset is NOT added: 8.7.2.5.5 uses cQpPicOffset), -12..12 */
    int cr_qp_offset;     /* pps_cr_qp_offset */
} hevcdbk_h265_params;

HEVCDBK_API size_t hevcdbk_h265_num_vert_bs(unsigned plane_w, unsigned plane_h); /* (plane_w/8+1) * (plane_h/4) */
HEVCDBK_API size_t hevcdbk_h265_num_hor_bs(unsigned plane_w, unsigned plane_h);  /* (plane_h/8+1) * (plane_w/4) */

/* per 4x4 luma unit prediction data the bS derivation (8.7.2.4) reads; (W/4) x (H/4) entries, row-major */
#define HEVCDBK_U_INTRA     0x0001u /* CuPredMode == MODE_INTRA */
#define HEVCDBK_U_CBF       0x0002u /* the luma transform block covering the unit has non-zero coefficient levels */
#define HEVCDBK_U_TU_LEFT   0x0004u /* the unit's left border is a transform block edge */
#define HEVCDBK_U_TU_TOP    0x0008u
#define HEVCDBK_U_PU_LEFT   0x0010u /* the unit's left border is a prediction block edge */
#define HEVCDBK_U_PU_TOP    0x0020u
#define HEVCDBK_U_KEEP      0x0040u /* samples stay unmodified (PCM + pcm_loop_filter_disabled_flag, transquant bypass) */
#define HEVCDBK_U_DBK_OFF   0x0080u /* slice_deblocking_filter_disabled_flag of the slice holding the unit */
#define HEVCDBK_U_PRED_L0   0x0100u /* predFlagL0: mv0 / ref0 valid */
#define HEVCDBK_U_PRED_L1   0x0200u
#define HEVCDBK_U_NOX_LEFT  0x0400u /* left border is a slice / tile boundary in-loop filtering must not cross */
#define HEVCDBK_U_NOX_TOP   0x0800u

typedef struct hevcdbk_h265_units {
    const uint16_t *flags;
    const int16_t *mv0;   /* [unit][2]: x, y in quarter luma samples */
    const int16_t *mv1;
    const int32_t *ref0;  /* identity of the reference PICTURE (e.g. its POC), not its index in the list */
    const int32_t *ref1;
} hevcdbk_h265_units;

/*
 * 8.7.2.4 on the GPU.  `units` and the four outputs are DEVICE pointers; the luma outputs have
 * hevcdbk_h265_num_vert_bs(w, h) / _hor_bs(w, h) entries, the chroma outputs (4:2:0, may both be NULL) those of the
 * (w/2) x (h/2) plane: the luma entry at twice the chroma position (8.7.2.5).  Asynchronous on `hip_stream`
 * (NULL = the context's compute stream).
 */
HEVCDBK_API int hevcdbk_h265_derive_bs_device(hevcdbk_context *ctx, const hevcdbk_h265_units *units, unsigned width, unsigned height,
                                  uint8_t *vert_bs4, uint8_t *hor_bs4, uint8_t *chroma_vert_bs4, uint8_t *chroma_hor_bs4,
                                  void *hip_stream);

/*
 * Spec-exact filter on planes that live in HBM.  `planes` as for hevc_deblocking_filter_device, except that vert_bs /
 * hor_bs are the 4-sample-granular arrays of THIS plane's geometry and qp_map / ctu_log2 describe QpY per unit of
 * (1 << ctu_log2) luma samples (3 = per 8x8, the finest a quantization group can be).  c_idx 0 = luma, 1 = Cb, 2 = Cr
 * (selects cb_qp_offset / cr_qp_offset; planes->is_chroma must agree).  The tables are the standard's (Table 8-12, 54 tc
 * entries); tc index = qPL + 2*(bS-1) + 2*tc_offset_div2, beta index = qPL + 2*beta_offset_div2, chroma through Table 8-10.
 * kernel_variant: HEVCDBK_KERNEL_AUTO, _GENERIC (32-bit arithmetic, every operand kind) or _PACKED (8-bit samples).
 */
HEVCDBK_API int hevc_deblocking_filter_h265_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, unsigned qp,
                                       const hevcdbk_h265_params *params, int kernel_variant, void *hip_stream);

/*
 * Host-frame operator of the spec-exact mode: uploads the frame and either `units` (HOST arrays; bS derived on the GPU)
 * or `bs4` (HOST luma arrays in the 4-sample-granular layout, n_vert / n_hor checked against hevcdbk_h265_num_*; the
 * chroma arrays are gathered from them on the GPU; its chroma_* members are ignored), filters Y and, when present, Cb and
 * Cr in place, downloads.  Exactly one of `units` / `bs4` must be non-NULL.  `qp` as for hevc_deblocking_filter.
 */
HEVCDBK_API int hevc_deblocking_filter_h265(hevcdbk_context *ctx, hevcdbk_frame *frame, const hevcdbk_h265_units *units,
                                const hevcdbk_bs *bs4, const hevcdbk_qp *qp, const hevcdbk_h265_params *params,
                                hevcdbk_timing *timing);

/* ==================================================================================================================
 * Sample adaptive offset, ITU-T H.265 clause 8.7.3: the in-loop stage that follows deblocking.  Not
 * present in the reference; parity against oracle/h265_oracle.c only ("parity unpinned").
 * ================================================================================================================== */
typedef struct hevcdbk_sao_ctb {
    uint8_t type;      /* SaoTypeIdx: 0 = not applied, 1 = band offset, 2 = edge offset */
    uint8_t cls;       /* band offset: sao_band_position (0..31); edge offset: SaoEoClass (0 hor, 1 ver, 2 135 deg, 3 45 deg) */
    int8_t offset[4];  /* SaoOffsetVal[1..4]: signed, already scaled by log2OffsetScale */
} hevcdbk_sao_ctb;

/*
 * SAO of planes that live in HBM, src -> dst (they must differ: the edge classifier reads deblocked neighbours).  Of
 * `planes` the members src, dst, pitch, frame_stride, n_frames, plane_w, plane_h (multiples of 8), bit_depth and
 * sample_bytes are used.  `params` (DEVICE memory): one entry per CTB of THIS plane, row stride params_stride entries,
 * params_frame_stride entries between frames (0 = shared); ctb_log2 = CTB size of this plane in samples (luma 4..6, 4:2:0
 * chroma one less: 3..5).  `keep` (DEVICE, may be NULL): one byte per 8x8 samples of this plane, non-zero = left
 * unmodified (PCM with pcm_loop_filter_disabled_flag, cu_transquant_bypass_flag), row stride keep_stride, frame stride
 * keep_frame_stride bytes.  Edge offset leaves a sample alone when one of its two neighbours is outside the picture.
 */
HEVCDBK_API int hevc_sao_filter_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params,
                           unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep,
                           unsigned keep_stride, size_t keep_frame_stride, void *hip_stream);

/*
 * Deblocking followed by SAO in ONE call, src -> dst (they must differ), of planes that live in HBM -- the in-loop chain of
 * a decoder.  Operands as for hevc_deblocking_filter_device (reference-exact mode: `qp`, `tables`, the
 * planes' bS arrays) resp. hevc_deblocking_filter_h265_device (spec-exact mode: `c_idx`, `qp`, `h265_params`, the planes'
 * 4-sample-granular bS arrays) and for hevc_sao_filter_device (`params` ... `keep_frame_stride`, all DEVICE memory).
 * For 8-bit planes and for 16-bit containers up to 12 bit, with one QP or a QP map, both stages run in ONE kernel: a workgroup
 * deblocks the offset blocks of a tile (8 bit: 192 x 128 samples, 16-bit containers: 128 x 128; plus a one-sample rim) into
 * LDS and applies SAO from there, so every sample is read from HBM once and written once and the deblocked picture never
 * exists in memory.  Other operands (samples deeper than 12 bit, misaligned 16-bit planes) run as two launches through a scratch plane owned
 * by the context.  `fused`: HEVCDBK_FUSED_AUTO picks, _OFF forces the two launches (same bytes; for A/B runs), _ON returns
 * HEVCDBK_ERR_UNSUPPORTED where the fused kernel does not apply.  The scratch plane of the two-launch form belongs to the
 * context and is reused by the next such call; its reuse is fenced by an event, so calls that hand in different streams are
 * ordered on it (like every entry point, a context serves one host thread at a time).  The fence holds after a call that
 * returned HEVCDBK_ERR_HIP as well: whatever that call had enqueued on its stream, the next call on any stream is ordered
 * behind it (where the event itself could not be recorded, the failing call waits for its stream instead).  A call blocks
 * the host only when the scratch has to grow: it then waits for the previous user before the buffer is freed.  The same
 * holds for the context's second scratch, the 4:2:2 SAO parameters of the _cf and later entries.  Parity: the deblocking stage as for
 * its own entry points; SAO against oracle/h265_oracle.c only ("parity unpinned").
 */
#define HEVCDBK_FUSED_AUTO 0
#define HEVCDBK_FUSED_OFF  1
#define HEVCDBK_FUSED_ON   2
HEVCDBK_API int hevc_deblock_sao_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp,
                                        const hevcdbk_tables *tables, const hevcdbk_sao_ctb *params, unsigned params_stride,
                                        size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride,
                                        size_t keep_frame_stride, int fused, void *hip_stream);
HEVCDBK_API int hevc_deblock_sao_h265_device(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, unsigned qp,
                                             const hevcdbk_h265_params *h265_params, const hevcdbk_sao_ctb *params,
                                             unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2,
                                             const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, int fused,
                                             void *hip_stream);

/*
 * The same for the planes of a 4:2:0 batch (other chroma formats: hevcdbk_h265_deblock_sao_device_planes_cf) -- planes[0] luma, the others chroma, n_planes <= 3, one frame count -- in ONE
 * call: where the fused kernel takes every plane (one sample width and bit depth) they go out as ONE launch, the planes'
 * tiles one after the other in the grid; otherwise plane by plane exactly as n_planes calls of the entries above would
 * (every plane is checked before the first launch).  sao[i] = the SAO operands of planes[i] (its own CTB grid: 4:2:0 chroma
 * has ctb_log2 one less than luma).  Spec-exact mode: c_idx = the plane's index (0 Y, 1 Cb, 2 Cr).  The reference has
 * neither stage after DeblockingFilter (main.cu:41-43) nor a multi-plane launch (gpu.cu:1269-1285: three launches).
 */
typedef struct {
    const hevcdbk_sao_ctb *params; /* DEVICE memory */
    unsigned params_stride;
    size_t params_frame_stride;
    unsigned ctb_log2;
    const uint8_t *keep;           /* DEVICE memory, may be NULL */
    unsigned keep_stride;
    size_t keep_frame_stride;
} hevcdbk_sao_plane;
HEVCDBK_API int hevc_deblock_sao_device_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                               unsigned qp, const hevcdbk_tables *tables, const hevcdbk_sao_plane *sao, int fused,
                                               void *hip_stream);
HEVCDBK_API int hevc_deblock_sao_h265_device_planes(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                                    unsigned qp, const hevcdbk_h265_params *h265_params,
                                                    const hevcdbk_sao_plane *sao, int fused, void *hip_stream);

/* ==================================================================================================================
 * Chroma formats of the spec-exact mode and SAO: 4:0:0, 4:2:0, 4:2:2, 4:4:4 (the RExt and Monochrome profiles).
 *
 * The entries above are the chroma_format_idc == 1 (4:2:0) case; the _cf entries below take the format as an operand
 * (HEVCDBK_CHROMA_* = chroma_format_idc) and, with HEVCDBK_CHROMA_420, produce exactly what the entries above produce.
 * SubWidthC x SubHeightC (Table 6-1) = 2x2 for 4:2:0, 2x1 for 4:2:2, 1x1 for 4:4:4; a chroma plane is
 * (W / SubWidthC) x (H / SubHeightC) and every rule is stated in its own sample coordinates:
 *   - chroma edges lie on the chroma plane's 8-sample grid (4:2:2: vertical edges every 16 luma columns, horizontal edges
 *     every 8 luma rows); the plane's bS arrays have the usual 4-sample-granular layout of ITS geometry, entry =
 *     the luma entry at (xDk * SubWidthC, yDm * SubHeightC) (8.7.2.5.5), only bS 2 filters;
 *   - QpQ / QpP = QpY of the unit covering luma sample (x * SubWidthC, y * SubHeightC);
 *   - QpC: Table 8-10 for 4:2:0, Min(qPi, 51) otherwise, qPi = ((QpQ + QpP + 1) >> 1) + cQpPicOffset (the pps offset
 *     only, for every format: CuQpOffsetC does not enter the deblocking);
 *   - SAO: the chroma CTB is (CtbSizeY / SubWidthC) x (CtbSizeY / SubHeightC): ctb_log2_w / ctb_log2_h (4:2:2 chroma:
 *     ctb_log2_h = ctb_log2_w + 1, e.g. 32 x 64 for CtbSizeY 64); params_stride counts CTB columns of that width;
 *     the keep map stays one byte per 8x8 samples of the plane;
 *   - 4:0:0: luma only; a chroma plane, c_idx > 0 or chroma bS outputs are HEVCDBK_ERR_ARG;
 *   - separate_colour_plane_flag = 1 (ChromaArrayType 0): each colour plane is coded as a monochrome picture, i.e. three
 *     luma calls (c_idx 0, HEVCDBK_CHROMA_400 or any format), each with its own bS, QP and SAO operands.
 * Kernels: every format, with one QP or a QP map, runs through the 32-bit kernel, the packed kernels and the fused
 * deblocking + SAO kernel -- Y, Cb, Cr of a 4:2:2 or 4:4:4 batch in ONE deblocking + SAO launch (4:2:2: after one small
 * launch that rewrites the chroma SAO parameters for square CTBs into a scratch owned by the context).  Parity: against a restatement of the standard in tests/, "parity
 * unpinned" as for the rest of the spec-exact mode.
 * ================================================================================================================== */
#define HEVCDBK_CHROMA_400 0
#define HEVCDBK_CHROMA_420 1
#define HEVCDBK_CHROMA_422 2
#define HEVCDBK_CHROMA_444 3

/* hevcdbk_h265_derive_bs_device for a picture of format chroma_format_idc: the chroma outputs (may both be NULL; must be
 * with 4:0:0) have the entry counts of the (width / SubWidthC) x (height / SubHeightC) plane */
HEVCDBK_API int hevcdbk_h265_derive_bs_device_cf(hevcdbk_context *ctx, const hevcdbk_h265_units *units, unsigned width,
                                                 unsigned height, int chroma_format_idc, uint8_t *vert_bs4, uint8_t *hor_bs4,
                                                 uint8_t *chroma_vert_bs4, uint8_t *chroma_hor_bs4, void *hip_stream);
/* hevc_deblocking_filter_h265_device for a plane of a picture of format chroma_format_idc (planes->plane_w / plane_h = this
 * plane's geometry; the QP map is indexed at (x * SubWidthC, y * SubHeightC)); kernel variants as there */
HEVCDBK_API int hevcdbk_h265_filter_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx,
                                                      int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *params,
                                                      int kernel_variant, void *hip_stream);
/* hevc_deblocking_filter_h265 for a frame of format chroma_format_idc: chroma planes (W / SubWidthC) x (H / SubHeightC),
 * multiples of 8 samples (else HEVCDBK_ERR_ARG; 4:2:0: HEVCDBK_ERR_DIMENSIONS as before); 4:0:0 frames carry no chroma
 * plane.  The chroma bS arrays are gathered from the luma arrays in the format's geometry */
HEVCDBK_API int hevcdbk_h265_filter_frame_cf(hevcdbk_context *ctx, hevcdbk_frame *frame, int chroma_format_idc,
                                               const hevcdbk_h265_units *units, const hevcdbk_bs *bs4, const hevcdbk_qp *qp,
                                               const hevcdbk_h265_params *params, hevcdbk_timing *timing);
/* hevc_sao_filter_device with CTBs of (1 << ctb_log2_w) x (1 << ctb_log2_h) samples: ctb_log2_h = ctb_log2_w (square) or
 * ctb_log2_w + 1 (4:2:2 chroma), 3..6 each */
HEVCDBK_API int hevcdbk_sao_filter_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params,
                                          unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w,
                                          unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                          size_t keep_frame_stride, void *hip_stream);
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx,
                                                int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride,
                                                unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                                size_t keep_frame_stride, int fused, void *hip_stream);
/* the planes of a batch in format chroma_format_idc (4:2:2 / 4:4:4: chroma planes in the format's geometry of planes[0], else
 * HEVCDBK_ERR_ARG; 4:2:0 with square CTBs: exactly hevc_deblock_sao_h265_device_planes); Y + Cb + Cr go out as ONE
 * deblocking + SAO launch where the fused kernel takes every plane, with one QP or a QP map */
typedef struct {
    const hevcdbk_sao_ctb *params; /* DEVICE memory */
    unsigned params_stride;
    size_t params_frame_stride;
    unsigned ctb_log2_w, ctb_log2_h;
    const uint8_t *keep;           /* DEVICE memory, may be NULL */
    unsigned keep_stride;
    size_t keep_frame_stride;
} hevcdbk_sao_plane_cf;
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_planes_cf(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                                       int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                       const hevcdbk_sao_plane_cf *sao, int fused, void *hip_stream);

/* ==================================================================================================================
 * SAO at slice and tile boundaries that in-loop filtering must not cross (ITU-T H.265 8.7.3.2).
 *
 * For a sample of an edge-offset CTB, edgeIdx is 0 -- the sample is copied -- when either of its two neighbours
 * (Table 8-13) lies outside the picture, OR belongs to a different slice and (the neighbour earlier in decoding order and
 * slice_loop_filter_across_slices_enabled_flag of the CURRENT sample's slice is 0, or the neighbour later and that flag of
 * the NEIGHBOUR's slice is 0), OR belongs to a different tile while loop_filter_across_tiles_enabled_flag is 0.  Slices and
 * tiles are made of whole CTBs, so every such boundary is a CTB border: the operand is one byte per CTB with one bit per
 * neighbouring CTB that this CTB's samples must not look into.  A CTB's byte speaks for the samples inside that CTB only
 * (it is never reconciled with the neighbour's byte); bits that point outside the picture are ignored; band offset, the
 * keep map and the picture-border rule are as in the entries above.  One CTB grid -- the luma one -- serves every plane of
 * a picture: the chroma CTBs are the luma CTBs sub-sampled.  Deblocking takes its share of the same syntax elements
 * through the units' HEVCDBK_U_NOX_LEFT / _TOP flags.  The reference has no SAO at all (main.cu:41-43 ends at
 * DeblockingFilter); parity against the per-sample restatement in tests/ only ("parity unpinned").  The meaning of the
 * bytes is tested on its own, independently of any slice / tile layout -- every byte value under every edge class, bytes
 * that contradict their neighbours' -- against tests/sao_borders_ref.py: sao_plane_by_bytes.
 * ================================================================================================================== */
#define HEVCDBK_SAO_NOX_L  0x01u /* the CTB left of this one must not be read by this CTB's samples */
#define HEVCDBK_SAO_NOX_R  0x02u
#define HEVCDBK_SAO_NOX_U  0x04u
#define HEVCDBK_SAO_NOX_D  0x08u
#define HEVCDBK_SAO_NOX_UL 0x10u
#define HEVCDBK_SAO_NOX_UR 0x20u
#define HEVCDBK_SAO_NOX_DL 0x40u
#define HEVCDBK_SAO_NOX_DR 0x80u
typedef struct hevcdbk_sao_borders { /* DEVICE memory; one CTB grid for all planes of a picture (the luma CTB grid) */
    const uint8_t *nox;              /* nox[cy * stride + cx] */
    unsigned stride;
    size_t frame_stride;             /* bytes between the frames of a batch, 0 = shared */
} hevcdbk_sao_borders;

/*
 * The bytes from what a decoder holds per CTB (DEVICE arrays, row stride in_stride entries): slice_idx = index of the CTB's
 * slice (not slice segment) in decoding order, slice_across = that slice's slice_loop_filter_across_slices_enabled_flag,
 * tile_idx = index of its tile (NULL = one tile).  One small launch, asynchronous like hevcdbk_h265_derive_bs_device;
 * callers that already hold the bits skip it.  Bits that point outside the picture come out 0.
 */
HEVCDBK_API int hevcdbk_h265_sao_borders_device(hevcdbk_context *ctx, const uint16_t *slice_idx, const uint8_t *slice_across,
                                                const uint16_t *tile_idx, int loop_filter_across_tiles_enabled_flag,
                                                unsigned ctbs_x, unsigned ctbs_y, unsigned in_stride, uint8_t *nox,
                                                unsigned nox_stride, void *hip_stream);
/*
 * The _cf entries with the operand.  borders == NULL is the _cf entry itself (the same launches); a non-NULL operand -- nox
 * non-NULL, stride at least the plane's CTB columns, else HEVCDBK_ERR_ARG -- runs the _nox twins of the same kernels, in
 * which a wave takes the masked form only where one of its lanes has a direction not to look in.  4:2:2 chroma (CTBs twice
 * as tall as wide): the bytes are rewritten for square CTBs together with the parameters.  The planes entry takes ONE
 * operand for the picture.
 */
HEVCDBK_API int hevcdbk_sao_filter_device_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params,
                                              unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w,
                                              unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                              size_t keep_frame_stride, const hevcdbk_sao_borders *borders, void *hip_stream);
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx,
                                                    int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                    const hevcdbk_sao_ctb *params, unsigned params_stride,
                                                    size_t params_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h,
                                                    const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride, int fused,
                                                    const hevcdbk_sao_borders *borders, void *hip_stream);
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_planes_nox(hevcdbk_context *ctx, const hevcdbk_device_planes *planes,
                                                           unsigned n_planes, int chroma_format_idc, unsigned qp,
                                                           const hevcdbk_h265_params *h265_params, const hevcdbk_sao_plane_cf *sao,
                                                           int fused, const hevcdbk_sao_borders *borders, void *hip_stream);

/* ==================================================================================================================
 * Per-slice deblocking offsets (ITU-T H.265 8.7.2.5.3 luma, 8.7.2.5.5 chroma).
 *
 * With deblocking_filter_override_enabled_flag a stream may set slice_beta_offset_div2 / slice_tc_offset_div2 in every slice, and
 * the standard takes both from the slice that holds sample q0,0 of each edge segment.  hevcdbk_h265_params carries one pair per
 * call; this operand carries one pair per CTB.  Rule: for every edge segment, luma and chroma, the beta and tC indices use the pair
 * of the CTB that holds the segment's q0,0; for a chroma plane that CTB is found at luma position (x * SubWidthC, y *
 * SubHeightC); chroma uses the tC offset only.  Slices are made of whole CTBs of at least 16 samples and edges lie on the 8-sample
 * grid, so one pair per CTB is exact.  With the operand present, tc_offset_div2 and beta_offset_div2 of hevcdbk_h265_params are
 * NOT USED (they are still range-checked); its cb_qp_offset / cr_qp_offset (cQpPicOffset) stay per call.  Values outside -6..6
 * are the caller's error: the indices are clipped as the standard clips them (0..51 and 0..53), so nothing is read out of range.
 * slice_deblocking_filter_disabled_flag goes through HEVCDBK_U_DBK_OFF, and slice_cb_qp_offset never enters deblocking.
 * Parity: against a composition of uniform-offset runs of the oracles in tests/ ("parity unpinned").
 * ================================================================================================================== */
typedef struct hevcdbk_h265_slice_offsets {  /* DEVICE memory; the LUMA CTB grid serves every plane of the picture */
    const int8_t *offs;    /* offs[2*(cy*stride+cx)] = slice_beta_offset_div2, [.. + 1] = slice_tc_offset_div2 of the slice holding the CTB;
                              2-byte aligned (a pair is read as one 16-bit word) */
    unsigned stride;       /* CTBs per row of the array, >= the picture's CTB columns */
    size_t frame_stride;   /* bytes between the frames of a batch, 0 = shared; a multiple of 2 */
    unsigned ctb_log2;     /* CtbLog2SizeY, 4..6 */
} hevcdbk_h265_slice_offsets;

/*
 * The pairs from what a decoder holds (DEVICE arrays): slice_idx = index of the CTB's slice in decoding order, one uint16_t per
 * CTB, row stride in_stride entries -- the array hevcdbk_h265_sao_borders_device takes; slice_table = int8_t[n_slices][2], beta
 * then tC.  A slice_idx >= n_slices yields (0, 0).  One small launch, asynchronous like its siblings; callers that already hold
 * the pairs skip it.  offs: 2 * offs_stride bytes per CTB row, 2-byte aligned.
 */
HEVCDBK_API int hevcdbk_h265_slice_offsets_device(hevcdbk_context *ctx, const uint16_t *slice_idx, unsigned in_stride,
                                                  const int8_t *slice_table, unsigned n_slices, unsigned ctbs_x, unsigned ctbs_y,
                                                  int8_t *offs, unsigned offs_stride, void *hip_stream);
/*
 * The _cf / _nox entries with the operand appended.  slice_offsets == NULL is the existing entry itself: the same kernels, grids
 * and blocks.  A non-NULL operand with offs == NULL (or misaligned), stride below the picture's CTB columns or ctb_log2 outside
 * 4..6 returns HEVCDBK_ERR_ARG before anything is enqueued.  With the operand every kernel family runs as its _sl twin -- the 32-bit
 * kernel, the packed kernels (8-bit and 16-bit containers) and the fused deblocking + SAO kernels, single plane and Y + Cb + Cr in
 * one launch -- for every chroma format, with one QP or a QP map, on the operands the family takes without it: kernel_variant and
 * `fused` mean what they mean there, and HEVCDBK_ERR_UNSUPPORTED comes back exactly where the entry without the operand returns
 * it.  The twins always run the per-lane (QP-map) form, a one-QP call with a constant qPL; no dummy map is needed.  `borders` of
 * the two deblocking + SAO entries may be NULL.  The planes entry takes ONE operand for the picture.  The host-frame operators
 * (hevc_deblocking_filter_h265, hevcdbk_h265_filter_frame_cf) and the reference-exact mode take no per-slice offsets.
 */
HEVCDBK_API int hevcdbk_h265_filter_device_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int chroma_format_idc,
                                              unsigned qp, const hevcdbk_h265_params *params, int kernel_variant,
                                              const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx,
                                                   int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                   const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride,
                                                   unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                                   size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                                   const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_planes_sl(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                                          int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                          const hevcdbk_sao_plane_cf *sao, int fused, const hevcdbk_sao_borders *borders,
                                                          const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* ==================================================================================================================
 * Planes sized in multiples of 4, not 8: the chroma planes of a 1920x1080 picture (the _g4 entries).
 *
 * An HEVC picture is a multiple of MinCbSizeY (>= 8) luma samples, so its 4:2:0 chroma planes are multiples of 4: 1920x1080 has
 * chroma planes of 960x540, and 540 = 67 * 8 + 4.  Every entry above demands multiples of 8 (plane_w % 8 == 0 && plane_h % 8 == 0, the
 * restriction stated for hevcdbk_device_planes) and keeps demanding them; the _g4 entries below have the SAME signatures as the
 * entries they extend and differ only in the plane sizes they accept.  A "g4 plane" has plane_w and plane_h that are multiples of 4
 * and at least 8.  Everything is stated in the plane's own sample coordinates:
 *   - the vertical edge x = 8k is filtered iff 0 < 8k < plane_w, the horizontal edge y = 8k iff 0 < 8k < plane_h.  For plane_w = 8k + 4
 *     the edge at x = 8k is an ordinary edge whose Q side is four samples wide: exactly the four samples 8.7.2.5 reads;
 *   - hevcdbk_h265_num_vert_bs / _num_hor_bs and the entry positions do not change ((W/8+1) x (H/4) and (H/8+1) x (W/4) with floor
 *     division): column plane_w/8 of the vertical array and row plane_h/8 of the horizontal array now hold a real edge.  Chroma
 *     entries are still the luma entry at (8 bx SubWidthC, 4 y4 SubHeightC) and its counterpart; only bS 2 filters;
 *   - QpY, QpC, KEEP_P / KEEP_Q, the offsets and slice_offsets (the CTB at the luma position of q0,0): as for every plane;
 *   - SAO: the CTB grid is ceil(plane / CTB) and the last CTB may be cut to a multiple of 4; the keep map has ceil(plane_w/8) bytes
 *     per row and ceil(plane_h/8) rows, the last byte of a row or column speaking for 4 samples; a sample whose edge-offset
 *     neighbour lies outside plane_w x plane_h is copied (8.7.3.2) -- which is why a caller cannot pad the planes to a multiple of
 *     8 instead: deblocking of the padded plane is right, SAO of its last row or column is not; band offset and `borders` as ever.
 * Accepted: the deblocking entries take g4 CHROMA planes (c_idx 1, 2) of 4:2:0, 4:2:2 and 4:4:4 pictures; a luma plane must stay
 * a multiple of 8 (HEVC produces nothing else) and returns HEVCDBK_ERR_DIMENSIONS.  The SAO entry takes any g4 plane.  A size that
 * is not a multiple of 4, or is below 8, returns HEVCDBK_ERR_DIMENSIONS before anything is enqueued.  With multiples of 8 a _g4 entry
 * IS the entry it extends: the same kernels, byte for byte.  A g4 plane runs the _g4 twins of the same kernel families -- the 32-bit
 * kernel, the packed kernels (8-bit and 16-bit containers, both block-to-lane maps), SAO (8-bit and 16-bit), the fused deblocking +
 * SAO kernels, single plane and Y + Cb + Cr in one launch -- under the same guards: kernel_variant and `fused` mean what they mean
 * there and HEVCDBK_ERR_UNSUPPORTED comes back where the multiple-of-8 call returns it.  The twins are built on the most general
 * forms (per-lane QP and per-slice offsets, boundary bytes), given neutral operands where the caller passes NULL.
 * The host-frame operators (hevc_deblocking_filter_h265, hevcdbk_h265_filter_frame_cf), the reference-exact mode (the reference
 * itself demands multiples of 8) and the file operators take no g4 planes.
 * Parity: tests/rext_oracle.py applied to the g4 plane, and for 4:2:0 the C oracle on the plane padded to a multiple of 8 and
 * cropped ("parity unpinned").
 * ================================================================================================================== */
/* like hevcdbk_h265_derive_bs_device_cf: width / height stay multiples of 8; the chroma arrays may be those of a g4 plane
 * (width / SubWidthC x height / SubHeightC, each at least 8, else HEVCDBK_ERR_DIMENSIONS) */
HEVCDBK_API int hevcdbk_h265_derive_bs_device_g4(hevcdbk_context *ctx, const hevcdbk_h265_units *units, unsigned width, unsigned height,
                                                 int chroma_format_idc, uint8_t *vert_bs4, uint8_t *hor_bs4, uint8_t *chroma_vert_bs4,
                                                 uint8_t *chroma_hor_bs4, void *hip_stream);
/* like hevcdbk_h265_filter_device_sl; slice_offsets may be NULL */
HEVCDBK_API int hevcdbk_h265_filter_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx, int chroma_format_idc,
                                              unsigned qp, const hevcdbk_h265_params *params, int kernel_variant,
                                              const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);
/* like hevcdbk_sao_filter_device_nox; borders may be NULL; keep_stride >= ceil(plane_w / 8) */
HEVCDBK_API int hevcdbk_sao_filter_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params,
                                             unsigned params_stride, size_t params_frame_stride, unsigned ctb_log2_w,
                                             unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                             size_t keep_frame_stride, const hevcdbk_sao_borders *borders, void *hip_stream);
/* like hevcdbk_h265_deblock_sao_device_sl; borders and slice_offsets may be NULL */
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, int c_idx,
                                                   int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                   const hevcdbk_sao_ctb *params, unsigned params_stride, size_t params_frame_stride,
                                                   unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep, unsigned keep_stride,
                                                   size_t keep_frame_stride, int fused, const hevcdbk_sao_borders *borders,
                                                   const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);
/* like hevcdbk_h265_deblock_sao_device_planes_sl; planes[0] (luma) is a multiple of 8 and the chroma planes are
 * planes[0] / (SubWidthC, SubHeightC), else HEVCDBK_ERR_ARG */
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_planes_g4(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned n_planes,
                                                          int chroma_format_idc, unsigned qp, const hevcdbk_h265_params *h265_params,
                                                          const hevcdbk_sao_plane_cf *sao, int fused, const hevcdbk_sao_borders *borders,
                                                          const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* ==================================================================================================================
 * Semi-planar chroma: one plane of interleaved Cb / Cr pairs (the _sp entries).
 *
 * Decoder surfaces are semi-planar: one Y plane and one plane whose rows hold Cb0 Cr0 Cb1 Cr1 ... (the NV12 layout, and its sibling
 * with 16-bit containers).  hevcdbk_h265_filter_device_sp deblocks such a chroma plane as it is, both components in one launch; a
 * caller need not split the pairs into two planes and merge them again.  hevcdbk_sao_filter_device_sp runs SAO on the same plane and
 * hevcdbk_h265_deblock_sao_device_sp the in-loop chain, deblocking then SAO: a decoder's chroma surface goes in and comes out as it
 * is.  4:2:0 only.
 *
 * The plane is described by a hevcdbk_device_planes with is_chroma = 1 (is_chroma = 0: HEVCDBK_ERR_ARG):
 *   - plane_w x plane_h are the samples PER COMPONENT (W/2 x H/2 of the picture); a row holds 2 * plane_w samples, the first
 *     component at the even positions, the second at the odd ones; pitch >= 2 * plane_w * sample_bytes, else HEVCDBK_ERR_ARG;
 *   - samples are LSB-aligned in their containers, like every plane here (P010 proper keeps its samples in the high bits: not taken);
 *   - plane_w and plane_h are multiples of 4 and at least 8 -- the rule of the _g4 entries, so the 960x540 pair plane of a 1920x1080
 *     picture is taken as it is -- else HEVCDBK_ERR_DIMENSIONS;
 *   - the bS arrays, the QP map and slice_offsets are those of the plane_w x plane_h chroma plane, exactly what the planar entries
 *     take, and both components use them (8.7.2 gives Cb and Cr of a 4:2:0 picture the same edges, the same QpY, the same slices and
 *     the same pcm / bypass flags).  What differs per component is cQpPicOffset.
 * NV21 order (Cr first) needs no flag: the caller swaps cb_qp_offset and cr_qp_offset.
 * The result is, per component, what hevcdbk_h265_filter_device_g4 gives for the split planes.
 * Alignment: pitch, frame_stride and both addresses are multiples of 4 * sample_bytes (else HEVCDBK_ERR_UNSUPPORTED), as for every
 * plane.  The packed kernels (HEVCDBK_KERNEL_PACKED, and HEVCDBK_KERNEL_AUTO where they apply) further need: samples of at most 12
 * bit; pitch, frame_stride and both addresses multiples of 8 bytes (8-bit samples) / 16 bytes (16-bit containers); plane_w < 8192
 * (one workgroup per block row); pitch * plane_h < 2^31.  Otherwise HEVCDBK_KERNEL_AUTO runs the 32-bit kernel and
 * HEVCDBK_KERNEL_PACKED returns HEVCDBK_ERR_UNSUPPORTED.  The packed kernels have the row map only: HEVCDBK_MAP_LINEAR returns
 * HEVCDBK_ERR_UNSUPPORTED.
 * Parity: tests/sp_ref.py -- the planar statement applied per component ("parity unpinned").
 * ================================================================================================================== */
/* like hevcdbk_h265_filter_device_g4, both components at once: no c_idx; params->cb_qp_offset applies to the even samples,
 * params->cr_qp_offset to the odd ones; slice_offsets may be NULL; src may equal dst */
HEVCDBK_API int hevcdbk_h265_filter_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp,
                                              const hevcdbk_h265_params *params, int kernel_variant,
                                              const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* SAO (8.7.3) of the pair plane described above, src -> dst (src == dst: HEVCDBK_ERR_ARG, as hevcdbk_sao_filter_device_g4 answers it).
 *   - params_cb speaks for the even samples of a row, params_cr for the odd ones (NV21: the caller swaps them; either NULL:
 *     HEVCDBK_ERR_ARG): two arrays with one stride and one frame stride, one entry per CTB of the plane_w x plane_h grid, taken by
 *     ceiling; the CTBs are square, ctb_log2 = 3..5 (else HEVCDBK_ERR_ARG);
 *   - keep is ONE map for both components, ceil(plane_w / 8) bytes per row (the flags behind it -- pcm with the loop filter disabled,
 *     transquant bypass -- belong to the coding unit); borders is ONE operand on the picture's CTB grid; either may be NULL.
 * The result is, per component, what hevcdbk_sao_filter_device_g4 gives for the split plane with that component's parameters -- for
 * ANY two entries of a CTB.  H.265 7.3.8.3 gives Cb and Cr of a CTB one SaoTypeIdx and one SaoEoClass with their own offsets and band
 * position; the kernels take a shorter path where the two agree, and are right where they do not.
 * The packed kernels run for samples of at most 12 bit when pitch, frame_stride and both addresses are multiples of a lane's row
 * piece -- 16 bytes (8-bit samples) / 32 bytes (16-bit containers) -- and pitch * plane_h < 2^31; every other plane takes the
 * per-sample kernel.  There is no kernel_variant.  Parity: tests/sao_sp_ref.py ("parity unpinned"). */
HEVCDBK_API int hevcdbk_sao_filter_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, const hevcdbk_sao_ctb *params_cb,
                                             const hevcdbk_sao_ctb *params_cr, unsigned params_stride, size_t params_frame_stride,
                                             unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                                             const hevcdbk_sao_borders *borders, void *hip_stream);

/* the in-loop chain on the pair plane: hevcdbk_h265_filter_device_sp (HEVCDBK_KERNEL_AUTO) into the context's scratch plane, then
 * hevcdbk_sao_filter_device_sp from there into dst -- two launches, a host composition.  fused: HEVCDBK_FUSED_AUTO and
 * HEVCDBK_FUSED_OFF run the two launches; HEVCDBK_FUSED_ON returns HEVCDBK_ERR_UNSUPPORTED before anything is enqueued (this entry
 * stays the host composition: the one-kernel form is hevcdbk_h265_deblock_sao_device_sp_fused below); any other value HEVCDBK_ERR_ARG */
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp,
                                                   const hevcdbk_h265_params *h265_params, const hevcdbk_sao_ctb *params_cb,
                                                   const hevcdbk_sao_ctb *params_cr, unsigned params_stride, size_t params_frame_stride,
                                                   unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride, size_t keep_frame_stride,
                                                   int fused, const hevcdbk_sao_borders *borders,
                                                   const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* The same chain in ONE kernel: a workgroup deblocks a tile of pairs into its LDS, the two components de-interleaved, and applies SAO
 * from there; the deblocked plane never exists in memory and the context's scratch plane is not touched.  Same operands as
 * hevcdbk_h265_deblock_sao_device_sp, same checks in the same order, and the result is byte for byte that entry's.
 * fused: HEVCDBK_FUSED_AUTO = the one-kernel form where the kernel's guards allow, else the two launches;
 *        HEVCDBK_FUSED_ON   = the one-kernel form, or HEVCDBK_ERR_UNSUPPORTED before anything is enqueued;
 *        HEVCDBK_FUSED_OFF  = the two launches; any other value HEVCDBK_ERR_ARG.
 * The guards: samples of at most 12 bit; pitch, frame_stride and both addresses multiples of a lane's row piece -- 16 bytes (8-bit
 * samples) / 32 bytes (16-bit containers); pitch * plane_h < 2^31; at most 65535 frames. */
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_sp_fused(hevcdbk_context *ctx, const hevcdbk_device_planes *planes, unsigned qp,
                                                         const hevcdbk_h265_params *h265_params, const hevcdbk_sao_ctb *params_cb,
                                                         const hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                                                         size_t params_frame_stride, unsigned ctb_log2, const uint8_t *keep,
                                                         unsigned keep_stride, size_t keep_frame_stride, int fused,
                                                         const hevcdbk_sao_borders *borders,
                                                         const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* SAO operands of a pair plane, as hevcdbk_sao_filter_device_sp takes them */
typedef struct hevcdbk_sao_plane_sp {
    const hevcdbk_sao_ctb *params_cb, *params_cr;
    unsigned params_stride;
    size_t params_frame_stride;
    unsigned ctb_log2; /* 3..5, square */
    const uint8_t *keep; /* may be NULL */
    unsigned keep_stride;
    size_t keep_frame_stride;
} hevcdbk_sao_plane_sp;

/* A whole semi-planar 4:2:0 picture -- the surface a decoder holds -- deblocked and SAO-filtered: luma (is_chroma = 0, sizes multiples
 * of 8) and pairs (is_chroma = 1, plane_w x plane_h per component = luma / 2, multiples of 4 and at least 8), the same n_frames,
 * sample_bytes and bit_depth (anything else: HEVCDBK_ERR_ARG).
 *   - Y is what hevcdbk_h265_deblock_sao_device_planes_g4 gives for the luma plane alone, the pair plane what
 *     hevcdbk_h265_deblock_sao_device_sp gives;
 *   - borders and slice_offsets are ONE operand each on the luma CTB grid, as for the _planes_g4 entry; either may be NULL;
 *   - sao_luma has square CTBs and sao_pairs->ctb_log2 == sao_luma->ctb_log2_w - 1, else HEVCDBK_ERR_ARG;
 *   - every operand of both planes is checked before the device is bound or anything is enqueued.
 * ONE launch when fused is not HEVCDBK_FUSED_OFF, both planes pass the guards of their fused kernels and both have the same kind of
 * QP (one value, or a map); otherwise plane by plane, each in its best available form.  HEVCDBK_FUSED_ON is refused with
 * HEVCDBK_ERR_UNSUPPORTED, before anything is enqueued, when a plane cannot be fused. */
HEVCDBK_API int hevcdbk_h265_deblock_sao_device_nv12(hevcdbk_context *ctx, const hevcdbk_device_planes *luma,
                                                     const hevcdbk_device_planes *pairs, unsigned qp,
                                                     const hevcdbk_h265_params *h265_params, const hevcdbk_sao_plane_cf *sao_luma,
                                                     const hevcdbk_sao_plane_sp *sao_pairs, int fused, const hevcdbk_sao_borders *borders,
                                                     const hevcdbk_h265_slice_offsets *slice_offsets, void *hip_stream);

/* ==================================================================================================================
 * SAO parameter estimation, the producing side of a codec: per-CTB statistics on the GPU and the choice of hevcdbk_sao_ctb from them.
 *
 * Every entry above APPLIES SAO parameters; these two PRODUCE them.  The chain is deblocking -> statistics -> pick -> SAO.
 *
 * Statistics, per sample of the deblocked plane `rec` against the original `org`:
 *   - a sample in a kept 8x8 block counts nowhere;
 *   - any other sample counts in its band bin, bo_*[rec >> (bitDepth - 5)];
 *   - such a sample counts in eo_*[k][e - 1] iff both neighbours of class k (Table 8-13) are available and its remapped edgeIdx
 *     (8.7.3.2: 0, 1, 2 -> 1, 2, 0) is e >= 1.  Available = inside the plane and, if in another CTB, not forbidden by the byte of the
 *     sample's own CTB, exactly as the boundary operand above defines the byte;
 *   - neighbour values are read whether or not the neighbour is kept, as SAO itself reads them.
 * So a sample counts in bin (class k, category e) if and only if hevcdbk_sao_filter_device_nox would add offset[e - 1] to it, were its
 * CTB an edge-offset CTB of class k under the same keep map and borders; likewise for the bands.  For any parameters, with n = count,
 * s = sum and o = offset, on inputs where the final clip to [0, max] never acts:
 *     SSE(org, SAO(rec)) - SSE(org, rec) = sum over the bins the parameters use of (n o^2 - 2 o s).
 * Parity: tests/sao_stats_ref.py, a per-sample statement, and that identity against the SAO statements ("parity unpinned").
 * ================================================================================================================== */
typedef struct hevcdbk_sao_stats {   /* one per CTB of THIS plane, 384 bytes, DEVICE memory */
    int32_t eo_count[4][4];          /* [SaoEoClass 0..3][edgeIdx - 1], edgeIdx 1..4 after the remap */
    int32_t eo_sum[4][4];            /* sum of (org - rec) over the counted samples */
    int32_t bo_count[32];            /* [rec >> (bitDepth - 5)] */
    int32_t bo_sum[32];
} hevcdbk_sao_stats;

/*
 * The statistics pass.  Of `rec` the members src (the deblocked plane: SAO's input), pitch, frame_stride, n_frames, plane_w, plane_h,
 * bit_depth (8..16) and sample_bytes are used; dst and the deblocking operands are not looked at.  `org` (DEVICE): the same geometry
 * and container with its own pitch and frame stride (bytes; a frame stride of 0 = one original for every frame, as for every operand).
 * plane_w and plane_h are multiples of 4 and at least 8 (else HEVCDBK_ERR_DIMENSIONS); the CTB grid and the keep map are taken by
 * ceiling as in the _g4 entries.  ctb_log2_w = 3..6, ctb_log2_h = ctb_log2_w or ctb_log2_w + 1 (4:2:2 chroma), at most 6.  keep and
 * borders may be NULL.  stats: stats_stride entries per CTB row (at least the CTB columns), stats_frame_stride entries between frames
 * (at least one grid when n_frames > 1: an output is never shared).  Every hevcdbk_sao_stats of the grid is written exactly once,
 * zeros included, with plain stores -- the caller clears nothing; entries beyond the CTB columns are not touched.  No global atomics:
 * the result is bit-reproducible.  All sums are exact in int32 (a 64x64 CTB at 16 bit reaches 4096 * 65535).  Rows that start at a
 * multiple of four samples in both planes move four samples per load; any other pitch or address that is a multiple of the sample
 * size runs sample by sample (a misaligned sample: HEVCDBK_ERR_UNSUPPORTED).  Any other bad operand: HEVCDBK_ERR_ARG.  Nothing is
 * enqueued on refusal.  Asynchronous on hip_stream (NULL = the context's compute stream).
 */
HEVCDBK_API int hevcdbk_sao_stats_device(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch,
                                         size_t org_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, const uint8_t *keep,
                                         unsigned keep_stride, size_t keep_frame_stride, const hevcdbk_sao_borders *borders,
                                         hevcdbk_sao_stats *stats, unsigned stats_stride, size_t stats_frame_stride, void *hip_stream);

/*
 * The statistics pass on a semi-planar chroma plane (NV12's second plane and its 16-bit sibling): `rec` and `org` are planes of
 * interleaved Cb / Cr pairs, and one launch fills one array per component.  The rule is that of hevcdbk_sao_stats_device per
 * component: stats_cb is, byte for byte, what hevcdbk_sao_stats_device gives for the plane of the even samples of every row with the
 * same keep map and the same borders, stats_cr the same for the odd samples.  A neighbour of a sample is the neighbouring PAIR's
 * sample of the same component, never the adjacent sample of the row.  The keep map is one byte per 8x8 pairs and serves both
 * components; borders is one byte per CTB of the per-component grid and serves both.  NV21 (Cr first) needs no flag: swap the outputs.
 *   - `rec` is described as every _sp entry describes a pair plane: is_chroma = 1; plane_w x plane_h per component, multiples of 4 and
 *     at least 8; pitch >= 2 * plane_w * sample_bytes, and org_pitch likewise; bit_depth 8..16 LSB-aligned.  Only src, the geometry and
 *     the container are looked at.  ctb_log2 = 3..5, square CTBs: the range of hevcdbk_sao_filter_device_sp.
 *   - stats_cb, stats_cr: two arrays with ONE stride and ONE frame stride (entries), the form hevcdbk_sao_pick_device reads (stats_a,
 *     stats_b).  Every entry of both grids is written exactly once, zeros included, with plain stores; entries beyond the CTB columns
 *     are not touched; with n_frames > 1 the frame stride is at least one grid.  No global atomics: the same bits every run.
 *   - org, keep, borders: a frame stride of 0 = shared, as everywhere.
 *   - Rows of both planes that start at a multiple of four pairs (bases, pitches and frame strides multiples of 8 * sample_bytes) take
 *     loads of four pairs; any other address or pitch that is a multiple of the sample size runs sample by sample.
 * Refusals, in this order, every one before the context is bound and with nothing enqueued: a NULL ctx, rec, rec->src, org, stats_cb or
 * stats_cr, a bad depth / container, is_chroma = 0 -- HEVCDBK_ERR_ARG; plane_w or plane_h no multiple of 4 or below 8 --
 * HEVCDBK_ERR_DIMENSIONS; then HEVCDBK_ERR_ARG for ctb_log2 outside 3..5, a pitch below two samples per pair, more than 65535 frames or
 * rows, a keep_stride below ceil(plane_w / 8), borders without bytes or with a stride below the CTB columns, a stats_stride below the
 * CTB columns, an output at an address that is no multiple of 4, a frame stride below one grid with n_frames > 1, and two outputs whose
 * extents (first entry to last) overlap; last, a sample at an address that is no multiple of its size -- HEVCDBK_ERR_UNSUPPORTED.
 * The chain of an NV12 picture's chroma: hevcdbk_h265_filter_device_sp -> this -> hevcdbk_sao_pick_device(stats_cb, stats_cr) ->
 * hevcdbk_sao_filter_device_sp(params_cb, params_cr).  Asynchronous on hip_stream (NULL = the context's compute stream).
 */
HEVCDBK_API int hevcdbk_sao_stats_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch,
                                            size_t org_frame_stride, unsigned ctb_log2, const uint8_t *keep, unsigned keep_stride,
                                            size_t keep_frame_stride, const hevcdbk_sao_borders *borders, hevcdbk_sao_stats *stats_cb,
                                            hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride,
                                            void *hip_stream);

/*
 * From statistics to parameters: the library's own rule, integers only, "parity unpinned" like the rest.
 * cost = deltaD * 256 + lambda_q8 * bits in int64, lambda_q8 <= 2^24 (else HEVCDBK_ERR_ARG); M = (1 << (Min(bitDepth, 10) - 5)) - 1;
 * log2OffsetScale is 0 in this entry; hevcdbk_sao_pick_device_os below takes it.
 *   - The offset of a bin (n, s): 0 if n = 0; otherwise o0 = sign(s) * ((2|s| + n) / (2n)), clamped to [0, M] for edge categories 1
 *     and 2, to [-M, 0] for categories 3 and 4 and to [-M, M] for bands; the search walks from o0 towards 0 one step at a time and
 *     keeps the o with the least (n o^2 - 2 o s) * 256 + lambda * bits(o), on a tie the one nearer 0;
 *     bits(o) = (|o| < M ? |o| + 1 : M), plus 1 sign bit for a non-zero band offset.
 *   - The candidates of a CTB, in this order, the lowest cost wins and on a tie the earliest: "not applied" costs lambda * 1; edge class
 *     0..3 costs lambda * 4 plus its four bins; band position 0..31 costs lambda * 7 plus the four bands (p + k) & 31.
 *   - stats_b != NULL (Cr beside Cb; params_b is then needed, and refused without it): both components share one type and one edge
 *     class and have their own offsets and band positions, as 7.3.8.3 demands.  "Not applied" costs lambda * 1; edge class c costs
 *     lambda * 4 plus both components' bins; band costs lambda * 2 plus, per component, lambda * 5 and its best position (on a tie
 *     the lowest).
 *   - delta_d (may be NULL): one int64 per CTB, tight -- [(frame * ctbs_y + cy) * ctbs_x + cx] -- the predicted change of the SSE
 *     under the choice, both components summed.
 * Both statistics arrays have one stride and one frame stride (entries), both parameter arrays likewise; params_frame_stride is at
 * least one grid when n_frames > 1.  ctbs_x, ctbs_y at least 1 (else HEVCDBK_ERR_DIMENSIONS).  One small launch, asynchronous.
 */
HEVCDBK_API int hevcdbk_sao_pick_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_a, const hevcdbk_sao_stats *stats_b,
                                        unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y,
                                        unsigned n_frames, unsigned bit_depth, unsigned lambda_q8, hevcdbk_sao_ctb *params_a,
                                        hevcdbk_sao_ctb *params_b, unsigned params_stride, size_t params_frame_stride, int64_t *delta_d,
                                        void *hip_stream);

/*
 * The same with log2_sao_offset_scale_luma / _chroma of the PPS range extension, k = log2_offset_scale: offsets are coded in units of
 * 2^k, so that at 11 and 12 bit they reach +-(31 << k) on samples that span 0..4095.  The operands of hevcdbk_sao_pick_device with
 * log2_offset_scale after bit_depth; the statistics do not change (band index rec >> (bitDepth - 5)).  Integers only; with
 * M = (1 << (Min(bitDepth, 10) - 5)) - 1 as above:
 *   - The offset of a bin (n, s) in coded units q: 0 if n = 0; otherwise q0 = sign(s) * ((2|s| + (n << k)) / (2 * (n << k))) -- the
 *     mean divided by 2^k, rounded half away from zero in ONE division, not round(s / n) >> k -- clamped to [0, M] for edge
 *     categories 1 and 2, to [-M, 0] for categories 3 and 4 and to [-M, M] for bands; the search walks from q0 towards 0 one step at
 *     a time and keeps the q with the least (n o^2 - 2 o s) * 256 + lambda * bits(q), where o = q * 2^k (a multiplication: a negative
 *     value is never shifted), on a tie the q nearer 0; bits is the bits(o) above, taken on the coded q.
 *   - The candidates of a CTB, their order, their side costs (lambda * 1, lambda * 4, lambda * 7, jointly lambda * 2 plus per
 *     component lambda * 5) and the tie rule (the earliest; in the joint form the band wins only when strictly less than everything
 *     before it) are exactly those above.  delta_d and every cost are taken on o.
 *   - params_a / params_b hold SaoOffsetVal = q * 2^k in offset[]: the SAO entries read them without change.
 *   - Range: n < 2^31 and |o| <= 124, so a bin's cost is below 2^54 and a CTB's below 2^58, in int64.
 *   - At k = 0 every output is byte for byte that of hevcdbk_sao_pick_device.  On the device the candidates of a CTB are compared
 *     by the lanes of a wave together, not walked by one lane; the result is the rule's, whichever entry runs.
 * Refusals: those of hevcdbk_sao_pick_device in its order -- NULL operands and pairing, then the depth, the lambda and, with them,
 * log2_offset_scale > Max(0, bit_depth - 10), which no stream codes -- HEVCDBK_ERR_ARG; the grid -- HEVCDBK_ERR_DIMENSIONS; strides,
 * addresses, the frame stride -- HEVCDBK_ERR_ARG; and LAST, before the context is bound and with nothing enqueued, a legal
 * log2_offset_scale > 2 -- HEVCDBK_ERR_UNSUPPORTED: it occurs at depths 13..16 only and needs offsets beyond int8_t (31 << 3 = 248).
 * Wide offsets on the applying side (hevcdbk_sao_ctb.offset[] is int8_t) are out of scope.
 */
HEVCDBK_API int hevcdbk_sao_pick_device_os(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_a, const hevcdbk_sao_stats *stats_b,
                                           unsigned stats_stride, size_t stats_frame_stride, unsigned ctbs_x, unsigned ctbs_y,
                                           unsigned n_frames, unsigned bit_depth, unsigned log2_offset_scale, unsigned lambda_q8,
                                           hevcdbk_sao_ctb *params_a, hevcdbk_sao_ctb *params_b, unsigned params_stride,
                                           size_t params_frame_stride, int64_t *delta_d, void *hip_stream);

/*
 * The SAO decision per CTB as 7.3.8.3 codes it: own parameters, sao_merge_left_flag or sao_merge_up_flag.  One flag takes the
 * neighbour's FINAL parameters of Y, Cb and Cr at once, so the decision is serial in raster order; on the device it runs along the
 * anti-diagonals of the CTB grid.  The chain is deblocking -> statistics -> decide -> SAO, nothing read back in between: for a planar
 * picture the three statistics arrays come from three hevcdbk_sao_stats_device calls, for NV12 from one such call (luma) and one
 * hevcdbk_sao_stats_device_sp call (stats_cb, stats_cr), and params_y / params_cb / params_cr are what hevcdbk_sao_filter_device_* /
 * _sp read.  The rule is the library's own, an extension of the pick rule above: integers only, "parity unpinned".
 *   - All three statistics arrays lie on ONE CTB grid (a chroma CTB grid has the luma grid's counts in every chroma format) with one
 *     stride and one frame stride (entries; 0 = shared).  stats_cb and stats_cr are both given or both NULL; both NULL is 4:0:0 or
 *     luma alone, and params_cb, params_cr, bit_depth_chroma and lambda_q8_chroma are then not looked at.
 *   - slice_idx, tile_idx: as hevcdbk_h265_sao_borders_device takes them, with one stride (idx_stride entries per CTB row) and one
 *     frame stride (entries; 0 = shared); either may be NULL = one slice / one tile.  A left candidate exists iff cx > 0 and the
 *     left CTB has the same slice index and the same tile index; an up candidate likewise with cy > 0.  For a conforming stream that
 *     is the condition of 7.3.8.3.  It is NOT the boundary byte of hevcdbk_sao_borders: slices with filtering across them enabled
 *     still do not merge.
 *   - pd(S, p) = the sum over the four bins p uses of n o^2 - 2 o s.  M_y, M_c: the pick rule's limit for each depth; both lambdas
 *     are at most 2^24.  The candidates of a CTB with statistics S_y, S_cb, S_cr, in this order:
 *       NEW   exactly what hevcdbk_sao_pick_device gives for S_y alone with lambda_q8_luma and for (S_cb, S_cr) jointly with
 *             lambda_q8_chroma; C_y, C_c = those picks' least costs (deltaD * 256 + lambda * bits); F = the number of candidates
 *             that exist (each flag coded as 0);
 *       LEFT  the left CTB's FINAL triple; C_y = 256 * pd(S_y, p_y), C_c = 256 * (pd(S_cb, p_cb) + pd(S_cr, p_cr)); F = 1;
 *       UP    the upper CTB's FINAL triple; C_y, C_c as for LEFT; F = 1 + (1 if a left candidate exists).
 *     The lowest J = lambda_c * C_y + lambda_l * C_c + lambda_l * lambda_c * F wins (D_y / lambda_l + D_c / lambda_c + R cleared of
 *     its divisions; without chroma J = C_y + lambda_l * F), on a tie the earliest.  J is compared exactly, in 128 bits.
 *   - params_*: the final triples, one stride and one frame stride; a merged CTB holds a copy of its neighbour's.
 *     log2_sao_offset_scale stays 0 (hevcdbk_sao_decide_device_os below takes it).  decision: the record below per CTB, its own stride and frame stride (entries).  Every entry of
 *     every output grid is written, with plain stores; entries beyond the CTB columns are not touched.  The same bits every run.
 *   - The slice-level slice_sao_luma_flag / slice_sao_chroma_flag are both taken as 1 here; hevcdbk_sao_slice_flags_device below
 *     chooses them per slice, and hevcdbk_sao_decide_device_sf decides under given ones.
 * Refusals, in this order, every one before the context is bound and with nothing enqueued: a NULL ctx, stats_y, params_y or
 * decision, exactly one of stats_cb / stats_cr, chroma statistics without params_cb or params_cr, a bit depth outside 8..16, a lambda
 * above 2^24 -- HEVCDBK_ERR_ARG; ctbs_x or ctbs_y of 0 or above 65535 -- HEVCDBK_ERR_DIMENSIONS; then HEVCDBK_ERR_ARG for a stride
 * (stats, params, decision; idx when an index array is given) below ctbs_x, a params_frame_stride or decision_frame_stride below one
 * grid with n_frames > 1, more than 65535 frames, statistics at an address that is no multiple of 4, a decision at one that is no
 * multiple of 8, an index array at an odd address, and an output whose extent (first entry to last) meets that of another output
 * or of a statistics array.  Two small launches, asynchronous on hip_stream (NULL = the context's compute stream).
 */
typedef struct hevcdbk_sao_decision {   /* one per CTB, 32 bytes, DEVICE memory */
    int64_t delta_d;      /* predicted change of the SSE under the FINAL parameters, the components summed */
    int64_t cost_luma;    /* C_y of the chosen candidate */
    int64_t cost_chroma;  /* C_c of the chosen candidate, 0 without chroma */
    uint8_t merge;        /* 0 = own parameters, 1 = sao_merge_left_flag, 2 = sao_merge_up_flag */
    uint8_t flag_bits;    /* F of the chosen candidate */
    uint8_t cand;         /* bit 0: a left candidate existed, bit 1: an up candidate existed */
    uint8_t zero[5];
} hevcdbk_sao_decision;

HEVCDBK_API int hevcdbk_sao_decide_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                          const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride,
                                          unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                                          unsigned bit_depth_chroma, unsigned lambda_q8_luma, unsigned lambda_q8_chroma,
                                          const uint16_t *slice_idx, const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride,
                                          hevcdbk_sao_ctb *params_y, hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr,
                                          unsigned params_stride, size_t params_frame_stride, hevcdbk_sao_decision *decision,
                                          unsigned decision_stride, size_t decision_frame_stride, void *hip_stream);

/*
 * The same with log2_sao_offset_scale_luma and log2_sao_offset_scale_chroma: the operands of hevcdbk_sao_decide_device with the two
 * scales after the two depths.  NEW is what hevcdbk_sao_pick_device_os gives for S_y alone with log2_offset_scale_luma and for
 * (S_cb, S_cr) jointly with log2_offset_scale_chroma; C_y, C_c are those picks' least costs.  LEFT and UP do not change: pd(S, p)
 * works on the stored, scaled offsets, so the merge walk along the anti-diagonals is the one above.  params_* hold
 * SaoOffsetVal = q * 2^k.  J stays below 2^83, inside the 128 bits it is compared in.  log2_offset_scale_chroma is not looked at
 * without chroma statistics.  At scales of 0 every output is byte for byte that of hevcdbk_sao_decide_device.
 * Refusals, in this order, every one before the context is bound and with nothing enqueued: those of hevcdbk_sao_decide_device up
 * to and including the depths and the lambdas, then a scale above Max(0, bit depth - 10) of its component -- HEVCDBK_ERR_ARG; the
 * grid -- HEVCDBK_ERR_DIMENSIONS; every further refusal of hevcdbk_sao_decide_device in its order -- HEVCDBK_ERR_ARG; and LAST a
 * legal scale above 2 (depths 13..16: offsets beyond int8_t) -- HEVCDBK_ERR_UNSUPPORTED.
 * What stays out: scales above 2 (wide offsets, on the applying side as well); a CABAC-accurate rate (bits() is the bin count of the
 * truncated unary code); the slice-level slice_sao_luma_flag / slice_sao_chroma_flag, both 1 here (hevcdbk_sao_decide_device_sf and
 * hevcdbk_sao_slice_flags_device below take and choose them); and routing
 * hevcdbk_sao_pick_device / hevcdbk_sao_decide_device to the kernels of the _os entries -- they keep their own.
 */
HEVCDBK_API int hevcdbk_sao_decide_device_os(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                             const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride,
                                             unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                                             unsigned bit_depth_chroma, unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma,
                                             unsigned lambda_q8_luma, unsigned lambda_q8_chroma, const uint16_t *slice_idx,
                                             const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride, hevcdbk_sao_ctb *params_y,
                                             hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                                             size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                             size_t decision_frame_stride, void *hip_stream);

/*
 * The decision under slice_sao_luma_flag / slice_sao_chroma_flag (7.3.6.1), which gate the sao() syntax of every CTB of a slice
 * (7.3.8.3): the operands of hevcdbk_sao_decide_device_os, then the flags before hip_stream.
 *   - slice_flags: DEVICE memory, one byte per slice of a frame, indexed by the value in slice_idx (slice_idx == NULL: every CTB is
 *     in slice 0); bit 0 = slice_sao_luma_flag (L), bit 1 = slice_sao_chroma_flag (C), higher bits ignored, bit 1 ignored without
 *     chroma statistics.  slice_flags_frame_stride: bytes between frames, 0 = shared.  A CTB whose slice_idx >= n_slices has flags 0
 *     (the convention of hevcdbk_h265_slice_offsets_device).  slice_flags == NULL is hevcdbk_sao_decide_device_os itself: the same
 *     launches, n_slices not looked at.
 *   - A CTB with L = C = 0: all three parameter entries are "not applied" (six zero bytes each) and its record is all zero -- no
 *     candidate exists, nothing is coded.  Otherwise the candidates and F are those of hevcdbk_sao_decide_device_os, but in NEW the
 *     luma part is that entry's luma pick only if L, else "not applied" with C_y = 0 (sao_type_idx_luma is not coded), and the chroma
 *     part is the joint Cb / Cr pick only if C, else both "not applied" with C_c = 0.  LEFT, UP, J, the tie rule and delta_d do
 *     not change: a candidate lies in the CTB's own slice and holds "not applied" where the flag is 0, so pd gives 0 there.
 *   - With every flag byte 3 the outputs are byte for byte those of hevcdbk_sao_decide_device_os.
 * Refusals: those of hevcdbk_sao_decide_device_os in its order, and with the stride checks n_slices of 0 or above 65536, with the
 * frame-stride checks a non-zero slice_flags_frame_stride below n_slices with n_frames > 1, with the extents slice_flags meeting an
 * output -- HEVCDBK_ERR_ARG; a legal scale above 2 stays LAST.  Two small launches, asynchronous on hip_stream.
 */
HEVCDBK_API int hevcdbk_sao_decide_device_sf(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                             const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride,
                                             unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                                             unsigned bit_depth_chroma, unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma,
                                             unsigned lambda_q8_luma, unsigned lambda_q8_chroma, const uint16_t *slice_idx,
                                             const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride, hevcdbk_sao_ctb *params_y,
                                             hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                                             size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                             size_t decision_frame_stride, const uint8_t *slice_flags, unsigned n_slices,
                                             size_t slice_flags_frame_stride, void *hip_stream);

/*
 * The flags chosen per slice, and the decision under them: filter -> statistics -> this call -> SAO yields on the device everything
 * 7.3.6.1 and 7.3.8.3 code for SAO, nothing read back.  The operands of hevcdbk_sao_decide_device_os, then n_slices, slice_flags
 * (OUTPUT, needed: [frame][slice], slice_flags_frame_stride bytes between frames), slice_record (OUTPUT, may be NULL: the record below
 * per slice and frame, its frame stride in entries) and the workspace: the caller's DEVICE memory, 16-byte aligned, of at least
 * hevcdbk_sao_slice_flags_workspace() bytes (a pure host function; about 150 bytes per CTB and frame); its contents afterwards
 * are unspecified.  The call allocates nothing and uses none of the context's scratch.
 *   - For a frame, a slice s < n_slices and a flag pair c = L + 2 C in {1, 2, 3}: T_c(s) = the sum, over the frame's CTBs whose slice
 *     index is s, of the chosen candidate's J in the decision of hevcdbk_sao_decide_device_sf with that slice's flags equal to c;
 *     T_0(s) = 0.  A merge candidate lies inside one slice, so T_c(s) depends on no other slice's flags and the best pair per slice
 *     is a minimum per slice.  The sums are exact: a CTB's J stays below 2^83, a total needs 128 bits (64 do not do: totals pass
 *     2^70 with statistics at the int32 ends and lambdas of 2^20 and 2^24).
 *   - The pair with the least T wins in the order 0, 1, 2, 3, on a tie the earliest -- the one that codes less.  Without chroma
 *     statistics only pairs 0 and 1 exist (cost entries 2 and 3 of the record are 0).  A slice with no CTB in the frame gets 0.
 *   - With chroma J is cleared of its divisions, so at lambdas of 0 every J is 0 and every slice ties to "no SAO": the degeneracy
 *     the decision itself has at a lambda of 0.
 *   - params_* and decision are then exactly what hevcdbk_sao_decide_device_sf writes under the chosen slice_flags.  Every entry of
 *     every output grid is written, with plain stores.  The same bits every run.
 * Refusals: those of hevcdbk_sao_decide_device_sf in its order (slice_flags_frame_stride, and slice_record's, below n_slices with
 * n_frames > 1: an output cannot be shared); then HEVCDBK_ERR_ARG for a NULL slice_flags, a NULL workspace or one at an address that
 * is no multiple of 16, workspace_bytes below the size function's value, a slice_record at an address that is no multiple of 8, and
 * slice_flags, slice_record or the workspace meeting another output or the statistics; a legal scale above 2 --
 * HEVCDBK_ERR_UNSUPPORTED; and LAST n_slices > 600 -- HEVCDBK_ERR_UNSUPPORTED: MaxSliceSegmentsPerPicture is 600 at the highest
 * levels, and the cap lets the totals of a frame live in LDS.  Three small launches, asynchronous on hip_stream.
 */
typedef struct hevcdbk_sao_slice_record {   /* one per slice and frame, 72 bytes, DEVICE memory */
    uint64_t cost_lo[4];  /* T_c as a 128-bit two's complement number, index = the flag pair c; entry 0 is 0 */
    int64_t  cost_hi[4];
    uint32_t n_ctbs;      /* CTBs of the frame with this slice index */
    uint8_t  flags;       /* the byte written to slice_flags */
    uint8_t  zero[3];
} hevcdbk_sao_slice_record;

HEVCDBK_API size_t hevcdbk_sao_slice_flags_workspace(unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned n_slices);

HEVCDBK_API int hevcdbk_sao_slice_flags_device(hevcdbk_context *ctx, const hevcdbk_sao_stats *stats_y, const hevcdbk_sao_stats *stats_cb,
                                               const hevcdbk_sao_stats *stats_cr, unsigned stats_stride, size_t stats_frame_stride,
                                               unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, unsigned bit_depth_luma,
                                               unsigned bit_depth_chroma, unsigned log2_offset_scale_luma, unsigned log2_offset_scale_chroma,
                                               unsigned lambda_q8_luma, unsigned lambda_q8_chroma, const uint16_t *slice_idx,
                                               const uint16_t *tile_idx, unsigned idx_stride, size_t idx_frame_stride, hevcdbk_sao_ctb *params_y,
                                               hevcdbk_sao_ctb *params_cb, hevcdbk_sao_ctb *params_cr, unsigned params_stride,
                                               size_t params_frame_stride, hevcdbk_sao_decision *decision, unsigned decision_stride,
                                               size_t decision_frame_stride, unsigned n_slices, uint8_t *slice_flags,
                                               size_t slice_flags_frame_stride, hevcdbk_sao_slice_record *slice_record,
                                               size_t slice_record_frame_stride, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Measured distortion: the sum of squared errors of a plane in HBM against the original, per CTB -- what the delta_d of the decision
 * and the totals of the slice records PREDICT, measured: the prediction equals the real change of the SSE only where the final clip
 * of SAO never acts, and deblocking has no prediction at all.  Nothing is read back: filter -> this call on the deblocked plane ->
 * SAO -> this call on SAO's output gives the distortion of every CTB before and after each stage, hevcdbk_sse_totals_device that of
 * every slice and frame (rate control, PSNR = one log10 on the host), all on the device.
 *   - rec and org mean what they mean to hevcdbk_sao_stats_device: of rec the members src, pitch, frame_stride, n_frames, plane_w,
 *     plane_h, bit_depth (8..16) and sample_bytes are used -- to measure an SAO output pass a descriptor whose src is that output;
 *     org has the same geometry with its own pitch and frame stride, a frame stride of 0 = one original for every frame.  plane_w
 *     and plane_h are multiples of 4 and at least 8; the CTB grid is taken by ceiling; ctb_log2_w 3..6, ctb_log2_h = ctb_log2_w or
 *     ctb_log2_w + 1 and at most 6.
 *   - sse[f * sse_frame_stride + cy * sse_stride + cx] = the sum of (org - rec)^2 over the samples of that CTB that lie inside the
 *     plane, exact (a 64 x 64 CTB at 16 bit reaches 4096 * 65535^2, about 2^44).  EVERY sample counts: there is no keep map and no
 *     borders operand -- a kept sample contributes equally before and after SAO.  Entries beyond the CTB columns are not touched;
 *     every entry of the grid is written once, with a plain store; no atomics; the same bits every run.
 *   - Rows that start at a multiple of 16 bytes in both planes (addresses, pitches and frame strides) are fetched 16 bytes per lane
 *     and load, rows at a multiple of four samples four samples per load, anything else sample by sample; the three give the same
 *     result.  No byte outside the plane_w x plane_h samples of a frame is read: the last row of the last frame may end the
 *     allocation.
 * Refusals, before the context is bound, in this order: NULL ctx / rec / rec->src / org / sse, a bad depth or sample_bytes --
 * HEVCDBK_ERR_ARG; the plane size -- HEVCDBK_ERR_DIMENSIONS; the CTB shape; a pitch below a row, more than 65535 frames or rows;
 * sse_stride below the CTB columns or above 0x7fffffff, sse at an address that is no multiple of 8; sse_frame_stride below one grid
 * with n_frames > 1 -- HEVCDBK_ERR_ARG; LAST a pitch, frame stride or address that is no multiple of the sample size --
 * HEVCDBK_ERR_UNSUPPORTED.  One launch, asynchronous on hip_stream (NULL = the context's compute stream).
 */
HEVCDBK_API int hevcdbk_sse_device(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch,
                                   size_t org_frame_stride, unsigned ctb_log2_w, unsigned ctb_log2_h, uint64_t *sse, unsigned sse_stride,
                                   size_t sse_frame_stride, void *hip_stream);

/*
 * The same of a plane of interleaved Cb / Cr pairs, described as for hevcdbk_sao_stats_device_sp: is_chroma = 1, plane_w x plane_h per
 * component, a pitch of at least two samples per pair, square CTBs of ctb_log2 3..5.  One launch fills both arrays: sse_cb is, byte
 * for byte, what hevcdbk_sse_device gives for the plane of the even samples, sse_cr the same for the odd samples (NV21: swap them),
 * with one stride and one frame stride.  Refusals: those of hevcdbk_sse_device in its order with what a pair plane replaces --
 * is_chroma beside the depth, the doubled pitch -- and, after the frame stride, two outputs whose extents meet: HEVCDBK_ERR_ARG.
 */
HEVCDBK_API int hevcdbk_sse_device_sp(hevcdbk_context *ctx, const hevcdbk_device_planes *rec, const void *org, size_t org_pitch,
                                      size_t org_frame_stride, unsigned ctb_log2, uint64_t *sse_cb, uint64_t *sse_cr,
                                      unsigned sse_stride, size_t sse_frame_stride, void *hip_stream);

/*
 * Per slice and per frame: sums of an array of the two entries above (or of any uint64_t per CTB).  slice_idx is what
 * hevcdbk_h265_sao_borders_device and the decision entries take (uint16_t per CTB, idx_stride entries per row, a frame stride of 0 =
 * shared); NULL = every CTB is in slice 0.  The chroma grids of every chroma format have the luma grid's counts, so the one luma
 * slice_idx serves each component's array: one call per component.
 *   - slice_total[f * slice_total_frame_stride + s], s < n_slices = the sum of the frame's entries whose slice index is s; a slice
 *     with no CTB gets 0.  frame_total[f] = the sum of ALL entries of the frame, CTBs whose index is >= n_slices included.  Either
 *     output may be NULL, not both.
 *   - Sums are modulo 2^64; on inputs from the entries above they never wrap (a frame has fewer than 2^32 samples).  One workgroup
 *     per frame, 64-bit integer adds in LDS -- they commute: the same bits every run; one plain store per output, no global atomics.
 * Refusals, in this order: NULL ctx / sse or both outputs NULL -- HEVCDBK_ERR_ARG; ctbs_x or ctbs_y of 0 or above 65535 --
 * HEVCDBK_ERR_DIMENSIONS; sse_stride (idx_stride with slice_idx) below ctbs_x or above 0x7fffffff; n_slices of 0 or above 65536; more
 * than 65535 frames; slice_total_frame_stride below n_slices with n_frames > 1; sse, slice_total or frame_total at an address that
 * is no multiple of 8, slice_idx of 2; outputs meeting each other or the input -- HEVCDBK_ERR_ARG; LAST n_slices > 600 --
 * HEVCDBK_ERR_UNSUPPORTED, the cap of hevcdbk_sao_slice_flags_device for the same reason.
 */
HEVCDBK_API int hevcdbk_sse_totals_device(hevcdbk_context *ctx, const uint64_t *sse, unsigned sse_stride, size_t sse_frame_stride,
                                          unsigned ctbs_x, unsigned ctbs_y, unsigned n_frames, const uint16_t *slice_idx,
                                          unsigned idx_stride, size_t idx_frame_stride, unsigned n_slices, uint64_t *slice_total,
                                          size_t slice_total_frame_stride, uint64_t *frame_total, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* HEVC_DEBLOCK_H */
