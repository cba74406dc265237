/*
 * sao_decide.hip -- the SAO decision per CTB on the producing side of a codec (hevcdbk_sao_decide_device): own parameters, merge left
 * or merge up over Y, Cb and Cr at once.  Not present in the reference.  The procedure is sao_decide.h; two launches on one stream.
 *
 * NEW (sao_decide_new_kernel): parallel, shaped like sao_pick_kernel -- one wave per CTB, lanes 0..47 choose the offset of one bin
 * each in every component, lane 0 the CTB's triple, its costs and the candidates that exist.
 *
 * MERGE (sao_decide_merge_kernel): the decision is serial in raster order -- a CTB's candidates are what its neighbours ENDED UP with
 * -- but the CTBs of one anti-diagonal d = cx + cy need only those of d - 1.  ONE workgroup of 256 threads per frame walks the
 * diagonals; its threads take a diagonal's CTBs in chunks of 256.  The finals of diagonal d - 1 are re-read from params_* in global
 * memory: they were written either by the NEW launch (an earlier kernel of the stream) or by threads of THIS workgroup before the
 * barrier that closes d - 1.  That barrier is __syncthreads(), a workgroup-scope release and acquire around s_barrier, behind an
 * explicit wait for every wave's outstanding stores; the waves of a workgroup share one CU and its L1, which is all workgroup scope
 * asks for.  No thread of any other workgroup ever touches this frame's entries.  Plain vector stores, no atomics.
 */
#include <hip/hip_runtime.h>

#include "sao_decide.h"
#include "sao_decide_launch.h"

namespace {

__global__ __launch_bounds__(64) void sao_decide_new_kernel(const DbkSaoDecideArgs a)
{
    __shared__ saostats::BinPick pk[3][saostats::kPickBins];
    const int lane = threadIdx.x, cx = blockIdx.x, cy = blockIdx.y, f = blockIdx.z;
    const long long at = ((long long)f * a.stats_frame_stride + (long long)cy * a.stats_stride + cx) * saostats::kBins;
    if (lane < saostats::kPickBins) {
        pk[0][lane] = saostats::pick_bin(a.stats_y + at, lane, a.max_offset_luma, a.lambda_luma);
        if (a.stats_cb) {
            pk[1][lane] = saostats::pick_bin(a.stats_cb + at, lane, a.max_offset_chroma, a.lambda_chroma);
            pk[2][lane] = saostats::pick_bin(a.stats_cr + at, lane, a.max_offset_chroma, a.lambda_chroma);
        }
    }
    __syncthreads();
    if (lane == 0) saodecide::new_ctb(a, f, cx, cy, pk[0], pk[1], pk[2]);
}

__global__ __launch_bounds__(saodecide::kChunk) void sao_decide_merge_kernel(const DbkSaoDecideArgs a)
{
    const int f = blockIdx.x, last = a.ctbs_x + a.ctbs_y - 2;
    for (int d = 1; d <= last; d++) { /* diagonal 0 is CTB (0, 0): no candidate */
        int cy0;
        const int n = saodecide::diagonal(a.ctbs_x, a.ctbs_y, d, cy0);
        for (int i = threadIdx.x; i < n; i += saodecide::kChunk) saodecide::merge_ctb(a, f, d - (cy0 + i), cy0 + i);
        if (d < last) { /* the same for every thread: d and last are uniform */
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
}

} /* namespace */

hipError_t dbk_launch_sao_decide(const DbkSaoDecideArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.ctbs_x <= 0 || a.ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_decide_new_kernel, dim3(a.ctbs_x, a.ctbs_y, a.n_frames), dim3(64), 0, stream, a);
    if (hipError_t e = hipGetLastError()) return e;
    return dbk_launch_sao_decide_merge(a, stream);
}

hipError_t dbk_launch_sao_decide_merge(const DbkSaoDecideArgs &a, hipStream_t stream)
{
    if (a.n_frames <= 0 || a.ctbs_x <= 0 || a.ctbs_y <= 0) return hipSuccess;
    if (a.ctbs_x + a.ctbs_y > 2) hipLaunchKernelGGL(sao_decide_merge_kernel, dim3(a.n_frames), dim3(saodecide::kChunk), 0, stream, a);
    return hipGetLastError();
}
