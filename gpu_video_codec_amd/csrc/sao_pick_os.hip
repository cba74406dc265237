/*
 * sao_pick_os.hip -- SAO parameter estimation with log2_sao_offset_scale (hevcdbk_sao_pick_device_os, hevcdbk_sao_decide_device_os).
 * Not present in the reference.  The procedure is sao_pick_os.h; the kernels of sao_stats.hip and sao_decide.hip stay as they are.
 *
 * Both kernels: a workgroup is ONE wave and owns one CTB.  Lanes 0..47 choose the offset of one bin each, per component in turn, into
 * LDS; then every lane forms the key of ITS candidate from those bins and the wave reduces to the least key with cross-lane moves:
 * no lane walks the candidates.  Lane 0 reads the winning candidate's four bins back and writes, with plain vector stores.
 *
 * The decision (sao_decide_new_os_kernel) writes what sao_decide_new_kernel writes -- the NEW triple and the whole record -- and is
 * followed on the same stream by sao_decide_merge_kernel of sao_decide.hip, unchanged: the merge costs are taken on the stored offsets.
 */
#include <hip/hip_runtime.h>

#include "sao_pick_os.h"
#include "sao_pick_os_launch.h"

namespace {

/* the least key of every group of WIDTH neighbouring lanes, in each of its lanes */
template <int WIDTH>
__device__ __forceinline__ saoos::Key group_min(saoos::Key k)
{
#pragma unroll
    for (int m = 1; m < WIDTH; m <<= 1) k = saoos::key_min(k, __shfl_xor(k, m));
    return k;
}

/* Cr (b) beside Cb (a): "not applied" and the edge classes in lanes 0..4, Cb's band positions in lanes 0..31 and Cr's in 32..63.  What
 * comes back is right in lane 0, which sits in the first group of each reduction and fetches Cr's least key from lane 32 */
__device__ __forceinline__ saoos::Choice joint(const saoos::BinPick *a, const saoos::BinPick *b, int lane, long long lambda)
{
    const saoos::Key edge = group_min<8>(saoos::joint_edge_key(a, b, lane, lambda));
    const saoos::Key band = group_min<32>(saoos::joint_band_key(a, b, lane));
    return saoos::joint_choice(edge, band, __shfl(band, 32), lambda);
}

__global__ __launch_bounds__(64) void sao_pick_os_kernel(const DbkSaoPickOsArgs o)
{
    __shared__ saoos::BinPick pk[2][saostats::kPickBins];
    const DbkSaoPickArgs &a = o.p;
    const int lane = threadIdx.x, cx = blockIdx.x, cy = blockIdx.y, f = blockIdx.z;
    const long long at = ((long long)f * a.stats_frame_stride + (long long)cy * a.stats_stride + cx) * saostats::kBins;
    if (lane < saostats::kPickBins) {
        pk[0][lane] = saoos::pick_bin(a.stats_a + at, lane, a.max_offset, o.log2_scale, a.lambda);
        if (a.stats_b) pk[1][lane] = saoos::pick_bin(a.stats_b + at, lane, a.max_offset, o.log2_scale, a.lambda);
    }
    __syncthreads();
    const saoos::Choice c = a.stats_b ? joint(pk[0], pk[1], lane, a.lambda) : saoos::single_choice(group_min<64>(saoos::single_key(pk[0], lane, a.lambda)));
    if (lane == 0) saoos::write_pick(a, f, cx, cy, pk[0], a.stats_b ? pk[1] : nullptr, c);
}

__global__ __launch_bounds__(64) void sao_decide_new_os_kernel(const DbkSaoDecideOsArgs o)
{
    __shared__ saoos::BinPick pk[3][saostats::kPickBins];
    const DbkSaoDecideArgs &a = o.d;
    const int lane = threadIdx.x, cx = blockIdx.x, cy = blockIdx.y, f = blockIdx.z;
    const long long at = ((long long)f * a.stats_frame_stride + (long long)cy * a.stats_stride + cx) * saostats::kBins;
    if (lane < saostats::kPickBins) {
        pk[0][lane] = saoos::pick_bin(a.stats_y + at, lane, a.max_offset_luma, o.log2_scale_luma, a.lambda_luma);
        if (a.stats_cb) {
            pk[1][lane] = saoos::pick_bin(a.stats_cb + at, lane, a.max_offset_chroma, o.log2_scale_chroma, a.lambda_chroma);
            pk[2][lane] = saoos::pick_bin(a.stats_cr + at, lane, a.max_offset_chroma, o.log2_scale_chroma, a.lambda_chroma);
        }
    }
    __syncthreads();
    const saoos::Choice y = saoos::single_choice(group_min<64>(saoos::single_key(pk[0], lane, a.lambda_luma)));
    saoos::Choice c = {};
    if (a.stats_cb) c = joint(pk[1], pk[2], lane, a.lambda_chroma); /* the same for every lane: a kernel operand */
    if (lane == 0) saoos::write_new(a, f, cx, cy, pk[0], pk[1], pk[2], y, c);
}

} /* namespace */

hipError_t dbk_launch_sao_pick_os(const DbkSaoPickOsArgs &a, hipStream_t stream)
{
    if (a.p.n_frames <= 0 || a.p.ctbs_x <= 0 || a.p.ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_pick_os_kernel, dim3(a.p.ctbs_x, a.p.ctbs_y, a.p.n_frames), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t dbk_launch_sao_decide_os(const DbkSaoDecideOsArgs &a, hipStream_t stream)
{
    if (a.d.n_frames <= 0 || a.d.ctbs_x <= 0 || a.d.ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_decide_new_os_kernel, dim3(a.d.ctbs_x, a.d.ctbs_y, a.d.n_frames), dim3(64), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    return dbk_launch_sao_decide_merge(a.d, stream);
}
