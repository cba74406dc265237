/*
 * hip_model.h -- a model of the HIP runtime for CPU tests of the host sources (csrc/deblock_host.cpp, csrc/deblock_host_h265.cpp,
 * csrc/deblock_host_sp.cpp), and of the kernel launchers above it: the host-frame operators (tests/host_frame_sim) and the device
 * entries that take the caller's stream (tests/device_stream_sim).  Unlike the stubs of tests/entry_sim, which complete
 * everything at once, the model DEFERS: a stream is a FIFO of operations, nothing runs when it is enqueued, and a scheduler
 * fixed per case decides inside which later HIP call an operation runs.  Streams are ordered against each other by
 * hipStreamWaitEvent on a recorded event and by nothing else.  Every behaviour here is one the real runtime may show.
 * What a kernel operation writes is decided when it RUNS, from what its operand arrays hold then: an operation that runs
 * before its operands were produced, or after they were overwritten, leaves other bytes than the test expects.
 *
 * Not modelled: time (hipEventElapsedTime answers 0 ms), the order of the DMA engines beyond stream order, and several
 * contexts or host threads sharing the runtime (hevcdbk_filter_yuv_file_multi).  hipFree waits for the device, as the
 * runtime's does: a buffer the code under test frees while work that uses it is queued is therefore never seen freed by that
 * work.  Growth of a context's scratch is checked for its results and for deadlock, not for use after free.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

enum ModelSched { SCHED_EAGER = 0, SCHED_LAZY = 1, SCHED_RANDOM = 2 };

/* the kinds of HIP call whose k-th occurrence a case can make fail */
enum ModelFault {
    FAULT_NONE = 0, FAULT_LAUNCH, FAULT_MEMCPY_ASYNC, FAULT_MEMCPY2D_ASYNC, FAULT_EVENT_RECORD, FAULT_STREAM_WAIT_EVENT,
    FAULT_EVENT_QUERY, FAULT_MALLOC, FAULT_HOST_MALLOC, FAULT_EXT_MALLOC, FAULT_KINDS
};
const char *model_fault_name(int kind);

struct ModelCase {
    int sched = SCHED_EAGER;
    uint32_t seed = 1;
    bool large_bar = true;
    bool supports = true;      /* what the *_supports predicates answer */
    bool push_unmapped = false; /* hipExtMallocWithFlags hands out an address with no mapping behind it: msync fails on it */
    int fault_kind = FAULT_NONE;
    int fault_at = 0; /* the k-th call of fault_kind returns an error (1-based) */
};

/* a new case: scheduler, faults and counters; allocations and registrations stay (a context may live on) */
void model_begin(const ModelCase &c);
/* counters of the calls so far in this case, by fault kind */
int model_calls(int kind);
/* violations recorded since model_begin: access checks, deadlocks, one line each */
const std::vector<std::string> &model_violations();
int model_sync_pageable_copies();
/* blocking calls since model_begin: hipStreamSynchronize, hipDeviceSynchronize, hipEventSynchronize; and hipFree of device memory */
int model_blocking_calls();
int model_device_frees();
/* what the *_supports predicates answer from now on (a session mixes calls the fused kernels take with calls they do not) */
void model_set_supports(bool supports);
/* operations still queued on any stream */
size_t model_pending_ops();
/* run everything that is queued (the test's own clean-up; not a HIP call of the code under test) */
void model_drain();

/* memory that hipHostRegister can map a second time: one memfd mapped twice.  The test takes planes from it; hipHostRegister of a
 * range inside it answers devicePointer = the alias, so a host address handed to a kernel is a different address and is caught */
void *model_region_alloc(size_t bytes);
void model_region_free(void *p);

/* the rows one kernel operation wrote: property (b) of the cases */
struct ModelWrite {
    const void *dst, *src; /* the plane's bases as the kernel was given them */
    int plane_h, frames;
    unsigned r0, r1;
};
const std::vector<ModelWrite> &model_writes();
/* the kind of memory behind a device-side address: 'd' hipMalloc, 'f' fine-grained, 'p' hipHostMalloc, 'r' registered, 0 none */
char model_kind_of(const void *dev_ptr);

/* ---- the marker arithmetic, shared by the launchers (what is in device memory when the operation runs) and by the test (what the
 * caller passed) ---- */
inline uint64_t model_fold(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
inline uint64_t model_fold_int(uint64_t h, long long v) { return model_fold(h, &v, sizeof v); }
inline uint64_t model_mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
/* never 0: a sample a kernel operation wrote differs from its input */
inline uint8_t model_m(uint64_t h, int chroma, unsigned y, unsigned x)
{
    const uint8_t v = (uint8_t)model_mix64(h + ((uint64_t)chroma << 62) + ((uint64_t)y << 24) + x);
    return v ? v : 0xA5;
}
/* what a launcher that produces operands writes over its whole output */
inline void model_derived(uint64_t h, uint8_t *out, size_t n)
{
    for (size_t i = 0; i < n; i++) out[i] = (uint8_t)model_mix64(h + i);
}
constexpr uint64_t kModelHash0 = 0xcbf29ce484222325ull;

/* ---- the SAO operations: a hash of the scalar operands and of every operand array, row by row of its grid (the bytes between
 * the rows of a strided array belong to nobody) ---- */
inline uint64_t model_fold_rows(uint64_t h, const void *base, size_t stride_bytes, size_t row_bytes, size_t rows)
{
    for (size_t r = 0; r < rows; r++) h = model_fold(h, (const uint8_t *)base + r * stride_bytes, row_bytes);
    return h;
}
inline uint64_t model_sao_hash0(int max_v, int band_shift, int ctb_log2)
{
    uint64_t h = kModelHash0 ^ 0x5a0;
    h = model_fold_int(h, max_v);
    h = model_fold_int(h, band_shift);
    return model_fold_int(h, ctb_log2);
}
/* the plane model_m takes for the SAO stage: deblocking uses 0 (luma) and 1 (chroma) */
constexpr int kModelSaoPlane = 2;
/* the launchers that produce operands (model_derived over their output) start their hash of the inputs here */
constexpr uint64_t kModelDeriveHash0 = kModelHash0 ^ 0xb5;
