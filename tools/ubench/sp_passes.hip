// sp_passes.hip -- what a caller of the PLANAR chroma entries pays around them when its surface is semi-planar (interleaved Cb / Cr
// pairs): the pass that splits the pairs into two planes, the pass that merges them again, and -- the yardstick -- a plain copy of
// the same bytes.  Every lane moves 16 bytes of the pair plane (8 pairs of 8-bit samples or 4 pairs of 16-bit containers).
//   sp_passes <samples per component across> <down> <frames> <sample bytes> [steps]
// One JSON line: ms per pass (median of 5 rounds of `steps` back-to-back launches).  Diagnostic only; not part of the product.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int SB> // pairs: n 16-byte pieces; cb, cr: 8 bytes each per piece
__global__ __launch_bounds__(256) void k_split(const uint4 *__restrict__ pairs, uint2 *__restrict__ cb, uint2 *__restrict__ cr, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 d = pairs[i];
    constexpr unsigned s0 = SB == 1 ? 0x06040200u : 0x05040100u, s1 = SB == 1 ? 0x07050301u : 0x07060302u;
    cb[i] = make_uint2(__builtin_amdgcn_perm(d.y, d.x, s0), __builtin_amdgcn_perm(d.w, d.z, s0));
    cr[i] = make_uint2(__builtin_amdgcn_perm(d.y, d.x, s1), __builtin_amdgcn_perm(d.w, d.z, s1));
}
template <int SB>
__global__ __launch_bounds__(256) void k_merge(const uint2 *__restrict__ cb, const uint2 *__restrict__ cr, uint4 *__restrict__ pairs, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 b = cb[i], r = cr[i];
    constexpr unsigned s0 = SB == 1 ? 0x05010400u : 0x05040100u, s1 = SB == 1 ? 0x07030602u : 0x07060302u;
    pairs[i] = make_uint4(__builtin_amdgcn_perm(r.x, b.x, s0), __builtin_amdgcn_perm(r.x, b.x, s1), __builtin_amdgcn_perm(r.y, b.y, s0),
                          __builtin_amdgcn_perm(r.y, b.y, s1));
}
__global__ __launch_bounds__(256) void k_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

template <typename F>
static double timed(F launch, int steps)
{
    std::vector<double> ms;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    for (int i = 0; i < 20; i++) launch();
    for (int r = 0; r < 5; r++) {
        hipEventRecord(e0, 0);
        for (int i = 0; i < steps; i++) launch();
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float t = 0.f;
        hipEventElapsedTime(&t, e0, e1);
        ms.push_back(t / steps);
    }
    std::sort(ms.begin(), ms.end());
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms[ms.size() / 2];
}

int main(int argc, char **argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s W H FRAMES SAMPLE_BYTES [STEPS]\n", argv[0]);
        return 2;
    }
    const size_t w = strtoul(argv[1], nullptr, 10), h = strtoul(argv[2], nullptr, 10), frames = strtoul(argv[3], nullptr, 10);
    const int sb = atoi(argv[4]), steps = argc > 5 ? atoi(argv[5]) : 100;
    const size_t bytes = 2 * w * h * frames * (size_t)sb, n = bytes / 16;
    if ((sb != 1 && sb != 2) || n == 0 || bytes % 16) return 2;
    uint4 *pairs, *back;
    uint2 *cb, *cr;
    CHECK(hipMalloc(&pairs, bytes));
    CHECK(hipMalloc(&back, bytes));
    CHECK(hipMalloc(&cb, bytes / 2));
    CHECK(hipMalloc(&cr, bytes / 2));
    CHECK(hipMemset(pairs, 0x5a, bytes));
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const double split = timed([&] { if (sb == 1) hipLaunchKernelGGL(k_split<1>, grid, block, 0, 0, pairs, cb, cr, n);
                                     else hipLaunchKernelGGL(k_split<2>, grid, block, 0, 0, pairs, cb, cr, n); }, steps);
    const double merge = timed([&] { if (sb == 1) hipLaunchKernelGGL(k_merge<1>, grid, block, 0, 0, cb, cr, back, n);
                                     else hipLaunchKernelGGL(k_merge<2>, grid, block, 0, 0, cb, cr, back, n); }, steps);
    const double copy = timed([&] { hipLaunchKernelGGL(k_copy, grid, block, 0, 0, pairs, back, n); }, steps);
    CHECK(hipDeviceSynchronize());
    printf("{\"pair_plane\": \"%zux%zu x %zu frames, %d-byte samples\", \"bytes\": %zu, \"split_ms\": %.4f, \"merge_ms\": %.4f, "
           "\"plain_copy_ms\": %.4f}\n", w, h, frames, sb, bytes, split, merge, copy);
    hipFree(pairs); hipFree(back); hipFree(cb); hipFree(cr);
    return 0;
}
