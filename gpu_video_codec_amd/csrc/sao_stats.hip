/*
 * sao_stats.hip -- SAO parameter estimation on the producing side of a codec: per-CTB statistics of a deblocked plane against the
 * original (hevcdbk_sao_stats_device) and the choice of hevcdbk_sao_ctb from them (hevcdbk_sao_pick_device).  Not present in the
 * reference.
 *
 * Statistics: a workgroup is ONE wave and owns one 64 x 64 region -- a whole number of CTBs at every allowed size -- of one frame;
 * a lane owns one 8 x 8 block of it (the keep map's unit, inside one CTB) and runs saostats::block on it.  The (bin, value) pairs
 * go into working histograms in LDS (saostats::kSlots 64-bit words: count low, sum high) with ONE 64-bit LDS add each; a CTB's
 * histogram is replicated by lane index so that the region holds at least 16 of them (a flat region -- every sample in one band
 * slot -- then has 4 lanes, not 64, on one address), 106 dwords apart so that the replicas of a slot lie in different banks.  After one barrier the lanes sum the replicas and write every int32 of the
 * region's CTBs once, with plain stores, zeros included: no global atomics, nothing to clear beforehand, the same bits every run.
 */
#include <hip/hip_runtime.h>

#include "sao_stats.h"
#include "sao_stats_launch.h"

namespace {

constexpr int kHistStride = saostats::kSlots + 1; /* 64-bit words: 106 dwords */

template <typename T>
struct Quad;
template <>
struct Quad<uint8_t> {
    using W = uint32_t;
    static __device__ __forceinline__ void unpack(W w, int *o) { o[0] = w & 0xff; o[1] = (w >> 8) & 0xff; o[2] = (w >> 16) & 0xff; o[3] = w >> 24; }
};
template <>
struct Quad<uint16_t> {
    using W = uint2;
    static __device__ __forceinline__ void unpack(W w, int *o) { o[0] = w.x & 0xffff; o[1] = w.x >> 16; o[2] = w.y & 0xffff; o[3] = w.y >> 16; }
};

/* VEC: every row of both planes starts at a multiple of four samples, so a lane moves four samples per load; otherwise sample by
 * sample (planes with an odd pitch in samples) */
template <typename T, bool VEC>
__global__ __launch_bounds__(64) void sao_stats_kernel(const DbkSaoStatsArgs a)
{
    extern __shared__ unsigned long long hist[];
    using W = typename Quad<T>::W;
    const int lane = threadIdx.x, bx = lane & 7, by = lane >> 3;
    const int x = (int)blockIdx.x * 64 + bx * 8, y0 = (int)blockIdx.y * 64 + by * 8, f = blockIdx.z;
    const int ncx = 64 >> a.lw, ncy = 64 >> a.lh, nctb = ncx * ncy;
    const int reps = nctb >= 16 ? 1 : 16 / nctb;
    for (int i = lane; i < nctb * reps * kHistStride; i += 64) hist[i] = 0;
    __syncthreads();
    if (x < a.plane_w && y0 < a.plane_h) {
        const bool kept = a.keep && a.keep[(long long)f * a.keep_frame_stride + (long long)(y0 >> 3) * a.keep_stride + (x >> 3)] != 0;
        if (!kept) {
            const saostats::Geo g = {a.plane_w, a.plane_h, a.lw, a.lh, a.band_shift};
            const uint32_t nox = a.nox ? a.nox[(long long)f * a.nox_frame_stride + (long long)(y0 >> a.lh) * a.nox_stride + (x >> a.lw)] : 0u;
            const int ctb = (((by * 8) >> a.lh) * ncx) + ((bx * 8) >> a.lw);
            const int rep = ((bx & 3) | ((by & 3) << 2)) & (reps - 1);
            unsigned long long *h = hist + (ctb * reps + rep) * kHistStride;
            const uint8_t *rec = a.rec + (long long)f * a.rec_frame_stride, *org = a.org + (long long)f * a.org_frame_stride;
            const int w = a.plane_w, hh = a.plane_h;
            const bool w8 = x + 8 <= w;
            auto ld_rec = [&](int y, int (&o)[10]) {
                const uint8_t *row = rec + (long long)(y < 0 ? 0 : (y >= hh ? hh - 1 : y)) * a.rec_pitch;
                if constexpr (VEC) {
                    int l[4], r[4];
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)x * sizeof(T)), &o[1]);
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(w8 ? x + 4 : x) * sizeof(T)), &o[5]); /* narrow: never used */
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x >= 4 ? x - 4 : 0) * sizeof(T)), l);
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(x + 12 <= w ? x + 8 : w - 4) * sizeof(T)), r);
                    o[0] = l[3];
                    o[9] = r[0];
                } else {
                    const T *s = reinterpret_cast<const T *>(row);
#pragma unroll
                    for (int i = 0; i < 10; i++) {
                        const int xx = x - 1 + i;
                        o[i] = s[xx < 0 ? 0 : (xx >= w ? w - 1 : xx)];
                    }
                }
            };
            auto ld_org = [&](int y, int (&o)[8]) {
                const uint8_t *row = org + (long long)y * a.org_pitch;
                if constexpr (VEC) {
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)x * sizeof(T)), &o[0]);
                    Quad<T>::unpack(*reinterpret_cast<const W *>(row + (size_t)(w8 ? x + 4 : x) * sizeof(T)), &o[4]);
                } else {
                    const T *s = reinterpret_cast<const T *>(row);
#pragma unroll
                    for (int i = 0; i < 8; i++) o[i] = s[x + i < w ? x + i : w - 1];
                }
            };
            /* count and sum of a slot are ONE 64-bit word -- count low, sum high -- and one ds_add_u64: the count stays below 2^32,
             * so nothing ever carries into the sum, and the high word adds d modulo 2^32, which is int32 addition */
            auto add = [&](int slot, int d) {
                __hip_atomic_fetch_add(h + slot, 1ull | ((unsigned long long)(uint32_t)d << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            if (saostats::needs_check(g, nox, x, y0)) saostats::block<true>(g, nox, x, y0, ld_rec, ld_org, add);
            else saostats::block<false>(g, nox, x, y0, ld_rec, ld_org, add);
        }
    }
    __syncthreads();
    const int ctbs_x = (a.plane_w + (1 << a.lw) - 1) >> a.lw, ctbs_y = (a.plane_h + (1 << a.lh) - 1) >> a.lh;
    for (int i = lane; i < nctb * saostats::kBins; i += 64) {
        const int c = i / saostats::kBins, bin = i - c * saostats::kBins;
        const int cy = c / ncx, cx = c - cy * ncx;
        const int gx = (int)blockIdx.x * ncx + cx, gy = (int)blockIdx.y * ncy + cy;
        if (gx >= ctbs_x || gy >= ctbs_y) continue;
        uint32_t v = 0;
        const int slot = saostats::bin_slot(bin); /* < kSlots: the count, the low half; else the sum of slot - kSlots, the high half */
        const int word = slot < saostats::kSlots ? slot : slot - saostats::kSlots, shift = slot < saostats::kSlots ? 0 : 32;
        for (int r = 0; r < reps; r++) v += (uint32_t)(hist[(c * reps + r) * kHistStride + word] >> shift);
        a.stats[((long long)f * a.stats_frame_stride + (long long)gy * a.stats_stride + gx) * saostats::kBins + bin] = (int32_t)v;
    }
}

/* One wave per CTB: lanes 0..47 choose the offset of one bin each (both components in turn), lane 0 the CTB's candidate */
__global__ __launch_bounds__(64) void sao_pick_kernel(const DbkSaoPickArgs a)
{
    __shared__ saostats::BinPick pk[2][saostats::kPickBins];
    const int lane = threadIdx.x, cx = blockIdx.x, cy = blockIdx.y, f = blockIdx.z;
    const long long at = ((long long)f * a.stats_frame_stride + (long long)cy * a.stats_stride + cx) * saostats::kBins;
    if (lane < saostats::kPickBins) {
        pk[0][lane] = saostats::pick_bin(a.stats_a + at, lane, a.max_offset, a.lambda);
        if (a.stats_b) pk[1][lane] = saostats::pick_bin(a.stats_b + at, lane, a.max_offset, a.lambda);
    }
    __syncthreads();
    if (lane != 0) return;
    DbkSaoCtb pa, pb;
    const long long dd = saostats::pick_ctb(pk[0], a.stats_b ? pk[1] : nullptr, a.lambda, pa, &pb);
    const long long out = (long long)f * a.params_frame_stride + (long long)cy * a.params_stride + cx;
    a.params_a[out] = pa;
    if (a.stats_b) a.params_b[out] = pb;
    if (a.delta_d) a.delta_d[((long long)f * a.ctbs_y + cy) * a.ctbs_x + cx] = dd;
}

} /* namespace */

bool dbk_sao_stats_vec(const DbkSaoStatsArgs &a, int sample_bytes)
{
    const size_t al = 4 * (size_t)sample_bytes;
    return (uintptr_t)a.rec % al == 0 && (uintptr_t)a.org % al == 0 && a.rec_pitch % (long long)al == 0 && a.org_pitch % (long long)al == 0 &&
           a.rec_frame_stride % (long long)al == 0 && a.org_frame_stride % (long long)al == 0;
}

hipError_t dbk_launch_sao_stats(const DbkSaoStatsArgs &a, int sample_bytes, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.plane_w <= 0 || a.plane_h <= 0) return hipSuccess;
    const dim3 grid((a.plane_w + 63) / 64, (a.plane_h + 63) / 64, a.n_frames), block(64);
    const int nctb = (64 >> a.lw) * (64 >> a.lh);
    const size_t lds = (size_t)(nctb >= 16 ? nctb : 16) * kHistStride * sizeof(unsigned long long);
    const bool vec = dbk_sao_stats_vec(a, sample_bytes);
    if (sample_bytes == 1) {
        if (vec) hipLaunchKernelGGL((sao_stats_kernel<uint8_t, true>), grid, block, lds, stream, a);
        else hipLaunchKernelGGL((sao_stats_kernel<uint8_t, false>), grid, block, lds, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((sao_stats_kernel<uint16_t, true>), grid, block, lds, stream, a);
        else hipLaunchKernelGGL((sao_stats_kernel<uint16_t, false>), grid, block, lds, stream, a);
    }
    return hipGetLastError();
}

hipError_t dbk_launch_sao_pick(const DbkSaoPickArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.ctbs_x <= 0 || a.ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_pick_kernel, dim3(a.ctbs_x, a.ctbs_y, a.n_frames), dim3(64), 0, stream, a);
    return hipGetLastError();
}
