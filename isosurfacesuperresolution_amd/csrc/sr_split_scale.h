// The scale rule of the split-operand scheme, in one place.  A tensor whose magnitude is not known in advance (a layer's weights, a
// gradient) is multiplied by 2^S before it is split into (hi, lo) fp16 pairs, with max |v| 2^S in [2^13, 2^14): hi stays far below the
// fp16 overflow and lo stays a normal number; the consumer undoes it exactly with 2^-S.  Every prepared weight image starts with the
// 16-byte header { 2^S, 2^-S, S, 0 }; the weight-gradient kernels keep the pair { 2^S, 2^-S } alone.
// Needs nothing of the split kernels' parameter blocks: sr_wgrad.hip includes it too.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// S = 13 - floor(log2(mx)), clamped to +-100; 0 for a maximum that is zero or not below 3e38 (infinite, NaN)
__device__ __forceinline__ int isr_scale_exponent(float mx)
{
    if (!(mx > 0.0f && mx < 3.0e38f)) return 0;
    const int S = 13 - ilogbf(mx);
    return S < -100 ? -100 : (S > 100 ? 100 : S);
}

__device__ __forceinline__ void isr_scale_pair(int S, float* pair)
{
    pair[0] = ldexpf(1.0f, S);
    pair[1] = ldexpf(1.0f, -S);
}

// header unit of a prepared weight image (16-byte aligned)
__device__ __forceinline__ void isr_scale_header(int S, void* image)
{
    uint4 hdr;
    hdr.x = __builtin_bit_cast(unsigned, ldexpf(1.0f, S));
    hdr.y = __builtin_bit_cast(unsigned, ldexpf(1.0f, -S));
    hdr.z = (unsigned)S; hdr.w = 0u;
    *reinterpret_cast<uint4*>(image) = hdr;
}

// the larger of two magnitudes, as floats or as their bit patterns; a NaN in `b` is dropped (as fmaxf does), `a` never becomes one
template <class T> __device__ __forceinline__ T isr_max(T a, T b) { return b > a ? b : a; }

// Maximum of `m` over the workgroup (whole waves, at most 1024 threads), returned to every thread.  A maximum is exact in any order.
// One use per kernel: a second one would need a barrier in front of it.
template <class T> __device__ __forceinline__ T isr_block_max(T m)
{
    __shared__ T red[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = isr_max(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    T r = red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = isr_max(r, red[k]);
    return r;
}

} // namespace
