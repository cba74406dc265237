/*
 * sao_slice.hip -- slice_sao_luma_flag / slice_sao_chroma_flag in SAO estimation (hevcdbk_sao_decide_device_sf,
 * hevcdbk_sao_slice_flags_device).  Not present in the reference.  The procedure is sao_slice.h; the kernels of sao_decide.hip and
 * sao_pick_os.hip stay as they are.
 *
 * NEW under given flags (sao_decide_new_sf_kernel): sao_decide_new_os_kernel's wave per CTB -- 48 lanes choose a bin's offset, every
 * lane forms the key of its candidate, the wave reduces -- whose lane 0 looks up the flag byte of the CTB's slice and masks the
 * components.  It is followed by sao_decide_merge_kernel of sao_decide.hip, unchanged.
 *
 * The choice, three launches on one stream:
 *   NEW (sao_slice_new_kernel): the same wave; lane 0 writes the two picks, computed ONCE, into the three states of the workspace.
 *   WALK (sao_slice_walk_kernel): ONE workgroup of 256 threads per frame walks the anti-diagonals; its threads take the (pair, CTB)
 *     items of a diagonal in chunks of 256.  As in sao_decide_merge_kernel the finals of diagonal d - 1 are re-read from global memory
 *     -- here from the workspace: they were written by the NEW launch (an earlier kernel of the stream) or by threads of THIS workgroup
 *     before the barrier that closes d - 1, which is __syncthreads(), a workgroup-scope release and acquire around s_barrier, behind
 *     an explicit wait for every wave's outstanding stores; the waves of a workgroup share one CU and its L1, which is all workgroup
 *     scope asks for.  No other workgroup touches this frame's states.  Each finished item adds its J, as 32-bit limbs, to 64-bit
 *     sums in LDS with LDS atomic adds: integer sums, the same in any order.  After the last barrier thread s propagates the carries
 *     of slice s, chooses and writes the flag byte and the record, with plain vector stores.
 *   FINAL (sao_slice_final_kernel): a thread per CTB copies the entries of the state its slice's flags name.  It is a launch of its
 *     own, not the tail of WALK: the flags are then read behind a kernel boundary and the copy of a 240 x 135 grid is spread over 127
 *     workgroups instead of 127 rounds of one.
 * No global atomics, nothing handed from workgroup to workgroup inside a launch, no spinning.
 */
#include <hip/hip_runtime.h>

#include "sao_slice.h"
#include "sao_slice_launch.h"

namespace {

/* the least key of every group of WIDTH neighbouring lanes, in each of its lanes (as in sao_pick_os.hip) */
template <int WIDTH>
__device__ __forceinline__ saoos::Key group_min(saoos::Key k)
{
#pragma unroll
    for (int m = 1; m < WIDTH; m <<= 1) k = saoos::key_min(k, __shfl_xor(k, m));
    return k;
}

__device__ __forceinline__ saoos::Choice joint(const saoos::BinPick *a, const saoos::BinPick *b, int lane, long long lambda)
{
    const saoos::Key edge = group_min<8>(saoos::joint_edge_key(a, b, lane, lambda));
    const saoos::Key band = group_min<32>(saoos::joint_band_key(a, b, lane));
    return saoos::joint_choice(edge, band, __shfl(band, 32), lambda);
}

/* the wave of sao_decide_new_os_kernel up to lane 0's write: the bins into pk, the two choices out */
__device__ __forceinline__ void picks(const DbkSaoDecideOsArgs &o, saoos::BinPick (&pk)[3][saostats::kPickBins], saoos::Choice &y, saoos::Choice &c)
{
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
    y = saoos::single_choice(group_min<64>(saoos::single_key(pk[0], lane, a.lambda_luma)));
    c = {};
    if (a.stats_cb) c = joint(pk[1], pk[2], lane, a.lambda_chroma); /* the same for every lane: a kernel operand */
}

__global__ __launch_bounds__(64) void sao_decide_new_sf_kernel(const DbkSaoSliceArgs s)
{
    __shared__ saoos::BinPick pk[3][saostats::kPickBins];
    saoos::Choice y, c;
    picks(s.o, pk, y, c);
    const int cx = blockIdx.x, cy = blockIdx.y, f = blockIdx.z;
    if (threadIdx.x == 0) saoslice::new_masked(s.o.d, f, cx, cy, pk[0], pk[1], pk[2], y, c, saoslice::pair_given(s, f, cx, cy));
}

__global__ __launch_bounds__(64) void sao_slice_new_kernel(const DbkSaoSliceArgs s)
{
    __shared__ saoos::BinPick pk[3][saostats::kPickBins];
    saoos::Choice y, c;
    picks(s.o, pk, y, c);
    if (threadIdx.x == 0) saoslice::new_states(s, blockIdx.z, blockIdx.x, blockIdx.y, pk[0], pk[1], pk[2], y, c);
}

__global__ __launch_bounds__(saodecide::kChunk) void sao_slice_walk_kernel(const DbkSaoSliceArgs s)
{
    extern __shared__ unsigned long long sums[]; /* n_slices x kSums, then n_slices counts of CTBs */
    unsigned *count = reinterpret_cast<unsigned *>(sums + (size_t)s.n_slices * saoslice::kSums);
    const DbkSaoDecideArgs &a = s.o.d;
    const int f = blockIdx.x, last = a.ctbs_x + a.ctbs_y - 2, n_pairs = saoslice::pairs(s);
    for (int i = threadIdx.x; i < s.n_slices * saoslice::kSums; i += saodecide::kChunk) sums[i] = 0;
    for (int i = threadIdx.x; i < s.n_slices; i += saodecide::kChunk) count[i] = 0;
    __syncthreads();
    for (int d = 0; d <= last; d++) { /* diagonal 0 is CTB (0, 0): no candidate, but a J */
        int cy0;
        const int n = saodecide::diagonal(a.ctbs_x, a.ctbs_y, d, cy0);
        for (int i = threadIdx.x; i < n * n_pairs; i += saodecide::kChunk) {
            const int pair = i / n + 1, k = i - (pair - 1) * n, cx = d - (cy0 + k), cy = cy0 + k;
            const unsigned sl = saoslice::slice_of(a, f, cx, cy);
            if (sl >= (unsigned)s.n_slices) continue; /* no candidate in any state: new_states */
            const saodecide::wide j = saoslice::walk_ctb(saoslice::pair_state(s, pair), f, cx, cy);
#pragma unroll
            for (int l = 0; l < 4; l++) atomicAdd(&sums[saoslice::sum_at(sl, pair, l)], (unsigned long long)saoslice::limb(j, l));
            if (pair == 1) atomicAdd(&count[sl], 1u);
        }
        if (d < last) { /* the same for every thread: d and last are uniform */
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    __syncthreads(); /* every sum is complete */
    for (int sl = threadIdx.x; sl < s.n_slices; sl += saodecide::kChunk) {
        DbkSaoSliceRecord rec;
        const unsigned flags = saoslice::choose(sums + (size_t)sl * saoslice::kSums, count[sl], a.stats_cb != nullptr, rec);
        s.flags_out[(long long)f * s.flags_frame_stride + sl] = (uint8_t)flags;
        if (s.record) s.record[(long long)f * s.record_frame_stride + sl] = rec;
    }
}

__global__ __launch_bounds__(256) void sao_slice_final_kernel(const DbkSaoSliceArgs s)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)s.o.d.ctbs_x * s.o.d.ctbs_y) return;
    saoslice::final_ctb(s, blockIdx.y, (int)(i % s.o.d.ctbs_x), (int)(i / s.o.d.ctbs_x));
}

} /* namespace */

hipError_t dbk_launch_sao_decide_sf(const DbkSaoSliceArgs &s, hipStream_t stream)
{
    const DbkSaoDecideArgs &a = s.o.d;
    if (a.n_frames <= 0 || a.ctbs_x <= 0 || a.ctbs_y <= 0) return hipSuccess;
    hipLaunchKernelGGL(sao_decide_new_sf_kernel, dim3(a.ctbs_x, a.ctbs_y, a.n_frames), dim3(64), 0, stream, s);
    if (hipError_t e = hipGetLastError()) return e;
    return dbk_launch_sao_decide_merge(a, stream);
}

hipError_t dbk_launch_sao_slice_flags(const DbkSaoSliceArgs &s, hipStream_t stream)
{
    const DbkSaoDecideArgs &a = s.o.d;
    if (a.n_frames <= 0 || a.ctbs_x <= 0 || a.ctbs_y <= 0) return hipSuccess;
    if (s.n_slices <= 0 || s.n_slices > saoslice::kMaxSlices) return hipErrorInvalidValue; /* the sums of a frame live in LDS */
    const size_t lds = (size_t)s.n_slices * (saoslice::kSums * sizeof(unsigned long long) + sizeof(unsigned));
    const long long n = (long long)a.ctbs_x * a.ctbs_y;
    hipLaunchKernelGGL(sao_slice_new_kernel, dim3(a.ctbs_x, a.ctbs_y, a.n_frames), dim3(64), 0, stream, s);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(sao_slice_walk_kernel, dim3(a.n_frames), dim3(saodecide::kChunk), lds, stream, s);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(sao_slice_final_kernel, dim3((unsigned)((n + 255) / 256), a.n_frames), dim3(256), 0, stream, s);
    return hipGetLastError();
}
