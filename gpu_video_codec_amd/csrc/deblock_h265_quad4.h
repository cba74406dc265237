/* deblock_h265_quad4.h -- 4 consecutive samples of a row as one memory word: the row access of the 32-bit kernels of the spec-exact
 * mode (deblock_h265.hip, deblock_sl.hip).  Internal to the translation unit that includes it. */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

template <typename T>
struct Quad4; /* 4 consecutive samples as one memory word */
template <>
struct Quad4<uint8_t> {
    using W = uint32_t;
    static __device__ __forceinline__ void unpack(W w, int &a, int &b, int &c, int &d)
    {
        a = w & 0xff; b = (w >> 8) & 0xff; c = (w >> 16) & 0xff; d = w >> 24;
    }
    static __device__ __forceinline__ W pack(int a, int b, int c, int d)
    {
        return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
    }
    static __device__ __forceinline__ W zero() { return 0u; }
};
template <>
struct Quad4<uint16_t> {
    using W = uint2;
    static __device__ __forceinline__ void unpack(W w, int &a, int &b, int &c, int &d)
    {
        a = w.x & 0xffff; b = w.x >> 16; c = w.y & 0xffff; d = w.y >> 16;
    }
    static __device__ __forceinline__ W pack(int a, int b, int c, int d)
    {
        return make_uint2((uint32_t)a | ((uint32_t)b << 16), (uint32_t)c | ((uint32_t)d << 16));
    }
    static __device__ __forceinline__ W zero() { return make_uint2(0u, 0u); }
};

} /* namespace */
