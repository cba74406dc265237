/*
 * sao_stats_sp.hip -- SAO parameter estimation on a semi-planar chroma plane: per-CTB statistics of a deblocked plane of interleaved
 * Cb / Cr pairs against an original of the same layout (hevcdbk_sao_stats_device_sp), one array of hevcdbk_sao_stats per component.
 * Not present in the reference.
 *
 * The shape is that of sao_stats.hip with a second wave: a workgroup is TWO waves and owns one region of 64 x 64 PAIRS -- 128 samples
 * by 64 rows, a whole number of CTBs at every allowed size -- of one frame; wave c owns component c (0 = the even samples), a lane of
 * it one 8 x 8 block of pairs, on which it runs saostats::block through the de-interleaving loaders of sao_stats_sp.h.  Keep flag,
 * CTB byte and histogram are per lane as in the planar kernel, and serve both waves.  Each component has its own set of working
 * histograms in LDS (saostats::kSlots 64-bit words, count low and sum high, ONE 64-bit LDS add per pair; at least 16 replicas per
 * region, 106 dwords apart).  After one barrier all 128 lanes sum the replicas and write every int32 of the region's CTBs once,
 * for both components, with plain stores: no global atomics, nothing to clear beforehand, the same bits every run.
 */
#include <hip/hip_runtime.h>

#include "sao_stats_sp.h"
#include "sao_stats_sp_launch.h"

namespace {

constexpr int kHistStride = saostats::kSlots + 1; /* 64-bit words: 106 dwords */

/* VEC: every row of both planes starts at a multiple of four pairs, so a lane moves four pairs per load; otherwise sample by sample */
template <typename T, bool VEC>
__global__ __launch_bounds__(128) void sao_stats_sp_kernel(const DbkSaoStatsSpArgs sp)
{
    extern __shared__ unsigned long long hist[];
    const DbkSaoStatsArgs &a = sp.p;
    const int tid = threadIdx.x, comp = tid >> 6, lane = tid & 63, bx = lane & 7, by = lane >> 3;
    const int x = (int)blockIdx.x * 64 + bx * 8, y0 = (int)blockIdx.y * 64 + by * 8, f = blockIdx.z;
    const int ncx = 64 >> a.lw, nctb = ncx * ncx;
    const int reps = nctb >= 16 ? 1 : 16 / nctb;
    const int per_comp = nctb * reps * kHistStride;
    for (int i = tid; i < 2 * per_comp; i += 128) hist[i] = 0;
    __syncthreads();
    if (x < a.plane_w && y0 < a.plane_h) {
        const bool kept = a.keep && a.keep[saostats_sp::keep_at(x, y0, a.keep_stride, a.keep_frame_stride, f)] != 0;
        if (!kept) {
            const saostats::Geo g = {a.plane_w, a.plane_h, a.lw, a.lw, a.band_shift};
            const uint32_t nox = a.nox ? a.nox[saostats_sp::nox_at(x, y0, a.lw, a.nox_stride, a.nox_frame_stride, f)] : 0u;
            const int ctb = (((by * 8) >> a.lw) * ncx) + ((bx * 8) >> a.lw);
            const int rep = ((bx & 3) | ((by & 3) << 2)) & (reps - 1);
            unsigned long long *h = hist + comp * per_comp + (ctb * reps + rep) * kHistStride;
            const saostats_sp::Plane rec = saostats_sp::frame_of(a.rec, a.rec_pitch, a.rec_frame_stride, f, a.plane_w, a.plane_h);
            const saostats_sp::Plane org = saostats_sp::frame_of(a.org, a.org_pitch, a.org_frame_stride, f, a.plane_w, a.plane_h);
            auto ld_rec = [&](int y, int (&o)[10]) { saostats_sp::ld_rec<T, VEC>(rec, comp, x, y, o); };
            auto ld_org = [&](int y, int (&o)[8]) { saostats_sp::ld_org<T, VEC>(org, comp, x, y, o); };
            /* count and sum of a slot are ONE 64-bit word, as in sao_stats.hip: the count stays below 2^32, nothing carries into the sum */
            auto add = [&](int slot, int d) {
                __hip_atomic_fetch_add(h + slot, 1ull | ((unsigned long long)(uint32_t)d << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            if (saostats::needs_check(g, nox, x, y0)) saostats::block<true>(g, nox, x, y0, ld_rec, ld_org, add);
            else saostats::block<false>(g, nox, x, y0, ld_rec, ld_org, add);
        }
    }
    __syncthreads();
    const int ctbs_x = (a.plane_w + (1 << a.lw) - 1) >> a.lw, ctbs_y = (a.plane_h + (1 << a.lw) - 1) >> a.lw;
    for (int i = tid; i < 2 * nctb * saostats::kBins; i += 128) {
        const int oc = i / (nctb * saostats::kBins), j = i - oc * nctb * saostats::kBins;
        const int c = j / saostats::kBins, bin = j - c * saostats::kBins;
        const int cy = c / ncx, cx = c - cy * ncx;
        const int gx = (int)blockIdx.x * ncx + cx, gy = (int)blockIdx.y * ncx + cy;
        if (gx >= ctbs_x || gy >= ctbs_y) continue;
        uint32_t v = 0;
        const int slot = saostats::bin_slot(bin); /* < kSlots: the count, the low half; else the sum of slot - kSlots, the high half */
        const int word = slot < saostats::kSlots ? slot : slot - saostats::kSlots, shift = slot < saostats::kSlots ? 0 : 32;
        for (int r = 0; r < reps; r++) v += (uint32_t)(hist[oc * per_comp + (c * reps + r) * kHistStride + word] >> shift);
        int32_t *out = oc ? sp.stats_cr : a.stats;
        out[((long long)f * a.stats_frame_stride + (long long)gy * a.stats_stride + gx) * saostats::kBins + bin] = (int32_t)v;
    }
}

} /* namespace */

size_t dbk_sao_stats_sp_lds(int ctb_log2)
{
    const int nctb = (64 >> ctb_log2) * (64 >> ctb_log2);
    return 2 * (size_t)(nctb >= 16 ? nctb : 16) * kHistStride * sizeof(unsigned long long);
}

bool dbk_sao_stats_sp_vec(const DbkSaoStatsSpArgs &sp, int sample_bytes)
{
    const DbkSaoStatsArgs &a = sp.p;
    const size_t al = 8 * (size_t)sample_bytes; /* four pairs */
    return (uintptr_t)a.rec % al == 0 && (uintptr_t)a.org % al == 0 && a.rec_pitch % (long long)al == 0 && a.org_pitch % (long long)al == 0 &&
           a.rec_frame_stride % (long long)al == 0 && a.org_frame_stride % (long long)al == 0;
}

hipError_t dbk_launch_sao_stats_sp(const DbkSaoStatsSpArgs &sp, int sample_bytes, hipStream_t stream)
{
    const DbkSaoStatsArgs &a = sp.p;
    if (a.n_frames <= 0 || a.plane_w <= 0 || a.plane_h <= 0) return hipSuccess;
    const dim3 grid((a.plane_w + 63) / 64, (a.plane_h + 63) / 64, a.n_frames), block(128);
    const size_t lds = dbk_sao_stats_sp_lds(a.lw); /* at most 54272 bytes: below the 64 KiB every kernel may ask for */
    const bool vec = dbk_sao_stats_sp_vec(sp, sample_bytes);
    if (sample_bytes == 1) {
        if (vec) hipLaunchKernelGGL((sao_stats_sp_kernel<uint8_t, true>), grid, block, lds, stream, sp);
        else hipLaunchKernelGGL((sao_stats_sp_kernel<uint8_t, false>), grid, block, lds, stream, sp);
    } else {
        if (vec) hipLaunchKernelGGL((sao_stats_sp_kernel<uint16_t, true>), grid, block, lds, stream, sp);
        else hipLaunchKernelGGL((sao_stats_sp_kernel<uint16_t, false>), grid, block, lds, stream, sp);
    }
    return hipGetLastError();
}
