/*
 * sse.hip -- measured distortion on the device: the sum of (org - rec)^2 per CTB of a plane (hevcdbk_sse_device), of both components
 * of a plane of interleaved Cb / Cr pairs (hevcdbk_sse_device_sp), and the sums of those per slice and per frame
 * (hevcdbk_sse_totals_device).  Not present in the reference.
 *
 * Per CTB: a workgroup is kWaves waves, a wave owns one region of 8 x 8 blocks of one frame -- a whole number of CTBs at every
 * allowed size -- and a lane one block of it, lane by * 8 + bx as in sao_stats.hip: 8 rows of 8 samples, of 16 samples on the
 * 16-byte path of an 8-bit plane (a region of 128 x 64), of 8 pairs on a pair plane.  The lane sums its block in registers
 * (sse::lane_sums), a CTB's sum is a butterfly over the lanes of that CTB (sse::butterfly), and one lane per CTB stores it.  The
 * kernels only read the planes: no LDS, no atomics, every output written once with a plain store, the same bits every run.
 *
 * Totals: one workgroup per frame; a lane walks its CTBs keeping the sum of the slice it is in (sse::totals_walk) and adds it to
 * the frame's array in LDS with one 64-bit integer add per run; one plain store per output.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sse.h"
#include "sse_launch.h"

namespace {

#ifndef DBK_SSE_WAVES
#define DBK_SSE_WAVES 4 /* measured: DESIGN 4.19 */
#endif
constexpr int kWaves = DBK_SSE_WAVES; /* waves of a workgroup of the per-CTB kernels, side by side in x */
constexpr int kTotalsThreads = 1024;

__device__ __forceinline__ unsigned long long lane_xor(unsigned long long v, int mask)
{
    const int lo = __shfl_xor((int)(uint32_t)v, mask, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
    return (unsigned long long)(uint32_t)lo | ((unsigned long long)(uint32_t)hi << 32);
}

/* PAIRS: a plane of interleaved pairs -- a lane's two sums are the even and the odd samples', each with its own output */
template <typename T, int MODE, bool ACC64, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void sse_kernel(const DbkSseArgs a)
{
    constexpr int NS = PAIRS ? 16 : (MODE == sse::kWide ? 16 / (int)sizeof(T) : 8); /* samples of a lane's row piece */
    constexpr int BW = PAIRS ? 8 : NS, BW_LOG2 = BW == 16 ? 4 : 3;                  /* its width in the units of plane_w */
    constexpr int SPLIT = PAIRS ? sse::kParity : (NS == 16 ? sse::kHalves : sse::kOne);
    using Acc = typename std::conditional<ACC64, unsigned long long, uint32_t>::type;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.z;
    const int rx = ((int)blockIdx.x * kWaves + wave) * 8 * BW, ry = (int)blockIdx.y * 64;
    const sse::Block b = sse::block_of(rx, ry, lane, BW, a.plane_w, a.plane_h);
    unsigned long long s[2];
    sse::lane_sums<T, MODE, NS, SPLIT, Acc>(a.rec + (long long)f * a.rec_frame_stride, a.org + (long long)f * a.org_frame_stride, a.rec_pitch,
                                            a.org_pitch, b, PAIRS ? 2 : 1, s);
    const int hs = sse::h_steps(a.lw, BW_LOG2), vs = sse::v_steps(a.lh);
    sse::fold<SPLIT>(a.lw, s);
    s[0] = sse::butterfly(s[0], hs, vs, lane_xor);
    if (sse::two_sums<SPLIT>(a.lw)) s[1] = sse::butterfly(s[1], hs, vs, lane_xor); /* both sums are somebody's: a component's, a CTB's */
    sse::store_ctbs<SPLIT>(lane, rx, ry, BW, a.plane_w, a.plane_h, a.lw, a.lh, hs, vs, s, [&](int which, int cx, int cy, unsigned long long v) {
        (which ? a.sse_odd : a.sse)[(long long)f * a.sse_frame_stride + (long long)cy * a.sse_stride + cx] = v;
    });
}

__global__ __launch_bounds__(kTotalsThreads) void sse_totals_kernel(const DbkSseTotalsArgs a)
{
    __shared__ unsigned long long tot[sse::kMaxSlices + 1]; /* the slices, then the frame */
    const int tid = threadIdx.x, f = blockIdx.x;
    for (int i = tid; i <= sse::kMaxSlices; i += kTotalsThreads) tot[i] = 0;
    __syncthreads();
    const uint16_t *idx = a.slice_idx ? a.slice_idx + (long long)f * a.idx_frame_stride : nullptr;
    auto flush = [&](int slice, unsigned long long v) { __hip_atomic_fetch_add(tot + slice, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    const unsigned long long all = sse::totals_walk(a.sse + (long long)f * a.sse_frame_stride, a.sse_stride, idx, a.idx_stride, a.ctbs_x, a.ctbs_y,
                                                    a.n_slices, tid >> 6, kTotalsThreads / 64, tid & 63, 64, flush);
    flush(sse::kMaxSlices, all);
    __syncthreads();
    if (a.slice_total)
        for (int s = tid; s < a.n_slices; s += kTotalsThreads) a.slice_total[(long long)f * a.slice_total_frame_stride + s] = tot[s];
    if (a.frame_total && tid == 0) a.frame_total[f] = tot[sse::kMaxSlices];
}

template <typename T, int MODE, bool PAIRS>
void launch(const DbkSseArgs &a, hipStream_t stream)
{
    constexpr int BW = PAIRS ? 8 : (MODE == sse::kWide ? 16 / (int)sizeof(T) : 8);
    const int regions = (a.plane_w + 8 * BW - 1) / (8 * BW);
    const dim3 grid((regions + kWaves - 1) / kWaves, (a.plane_h + 63) / 64, a.n_frames), block(64 * kWaves);
    if (sizeof(T) == 2 && a.wide_acc) hipLaunchKernelGGL((sse_kernel<T, MODE, sizeof(T) == 2, PAIRS>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((sse_kernel<T, MODE, false, PAIRS>), grid, block, 0, stream, a);
}

template <bool PAIRS>
hipError_t launch_any(const DbkSseArgs &a, int sample_bytes, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.plane_w <= 0 || a.plane_h <= 0) return hipSuccess;
    const int mode = dbk_sse_mode(a, sample_bytes);
    if (sample_bytes == 1) {
        if (mode == sse::kWide) launch<uint8_t, sse::kWide, PAIRS>(a, stream);
        else if (mode == sse::kQuad) launch<uint8_t, sse::kQuad, PAIRS>(a, stream);
        else launch<uint8_t, sse::kScalar, PAIRS>(a, stream);
    } else {
        if (mode == sse::kWide) launch<uint16_t, sse::kWide, PAIRS>(a, stream);
        else if (mode == sse::kQuad) launch<uint16_t, sse::kQuad, PAIRS>(a, stream);
        else launch<uint16_t, sse::kScalar, PAIRS>(a, stream);
    }
    return hipGetLastError();
}

} /* namespace */

int dbk_sse_mode(const DbkSseArgs &a, int sample_bytes)
{
    auto all = [&](long long al) {
        return (uintptr_t)a.rec % al == 0 && (uintptr_t)a.org % al == 0 && a.rec_pitch % al == 0 && a.org_pitch % al == 0 && a.rec_frame_stride % al == 0 &&
               a.org_frame_stride % al == 0;
    };
    return all(16) ? sse::kWide : (all(4 * sample_bytes) ? sse::kQuad : sse::kScalar);
}

hipError_t dbk_launch_sse(const DbkSseArgs &a, int sample_bytes, hipStream_t stream) { return launch_any<false>(a, sample_bytes, stream); }
hipError_t dbk_launch_sse_sp(const DbkSseArgs &a, int sample_bytes, hipStream_t stream) { return launch_any<true>(a, sample_bytes, stream); }

hipError_t dbk_launch_sse_totals(const DbkSseTotalsArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0) return hipSuccess;
    hipLaunchKernelGGL(sse_totals_kernel, dim3(a.n_frames), dim3(kTotalsThreads), 0, stream, a);
    return hipGetLastError();
}
