// The temporal input path's arithmetic, shared by the inference kernels (sr_frame.hip) and the training kernels (sr_train.hip).
#pragma once
#include <hip/hip_runtime.h>

// The temporal input path -- flow hole filling, resize of the flow, warp of the previous frame -- is DEFINED operation by operation in
// the package's module path (inference/flowfill.py, models/videotools.py: elementwise torch operations, one IEEE rounding each) and
// computed here with the same operations in the same order and NO contraction into FMAs (`#pragma clang fp contract(off)` in every
// function that takes part): same inputs, same bits.  Why it matters: the reference's warp goes through normalised coordinates, a
// rounding of 6e-8 there is 6e-5 pixels at 1080p and 1e-4 in the warped value across a silhouette edge; two fp32 evaluations that
// round differently hand the network inputs that differ by that much, and the recurrence multiplies it frame by frame
// (tests/test_recurrence_gpu.py, DESIGN "temporal input path").
__device__ __forceinline__ void isr_src_index_rn(int dst, float scale, int in_size, int& i0, int& i1, float& l1)
{
#pragma clang fp contract(off)
    float s = ((float)dst + 0.5f) * scale;      // (dst + 0.5) * scale - 0.5, clamped at 0 (ATen area_pixel_compute_source_index)
    s = s - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

// hy (hx a + lx b) + ly (hx c + lx d): seven roundings in this order (models/videotools.py: bilinear_taps)
__device__ __forceinline__ float isr_bilerp_rn(float hy, float hx, float ly, float lx, float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    const float ha = hx * a, lb = lx * b, hc = hx * c, ld = lx * d;
    const float t0 = ha + lb, t1 = hc + ld;
    const float u0 = hy * t0, u1 = ly * t1;
    return u0 + u1;
}

// linspace(-1, 1, n)[i] as models/videotools.py: pixel_grid defines it: 2 i / (n - 1) - 1 in double (multiply, divide, subtract),
// rounded once to float
__device__ __forceinline__ float isr_pixel_grid(int i, int n)
{
#pragma clang fp contract(off)
    const double twice = (double)i * 2.0;
    const double q = twice / (double)(n > 1 ? n - 1 : 1);
    return (float)(q - 1.0);
}


// Where VideoTools.warp_upscale(., flow, 4) samples the previous frame for the high-resolution pixel (X, Y), operation by operation as
// models/videotools.py spells it out (and as assemble_input_kernel does for the unshaded networks): the flow scaled by (-2, +2), resized
// x4 (align_corners=False), added to the pixel grid; sampler with align_corners=True and zero padding.  b00 = iy0 W + ix0 is the first
// tap, v* say which of the four taps lie inside the image, w* are their weights; the caller adds ((v00 w00 + v01 w01) + v10 w10) + v11 w11.
struct IsrWarpTaps {
    long long b00;
    int ix0, iy0;
    bool vx0, vx1, vy0, vy1;
    float w00, w01, w10, w11;
};

__device__ __forceinline__ IsrWarpTaps isr_warp_taps(const float* fx, const float* fy, int h, int w, int X, int Y)
{
#pragma clang fp contract(off)
    const int H = 4 * h, W = 4 * w;
    const float sx_scale = 0.5f * (float)(W - 1), sy_scale = 0.5f * (float)(H - 1);
    int y0, y1, x0, x1; float ly, lx;
    isr_src_index_rn(Y, 0.25f, h, y0, y1, ly);
    isr_src_index_rn(X, 0.25f, w, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float flx = isr_bilerp_rn(hy, hx, ly, lx, fx[y0 * w + x0] * -2.0f, fx[y0 * w + x1] * -2.0f, fx[y1 * w + x0] * -2.0f, fx[y1 * w + x1] * -2.0f);
    const float fly = isr_bilerp_rn(hy, hx, ly, lx, fy[y0 * w + x0] * 2.0f, fy[y0 * w + x1] * 2.0f, fy[y1 * w + x0] * 2.0f, fy[y1 * w + x1] * 2.0f);
    const float gx = isr_pixel_grid(X, W) + flx;
    const float gy = isr_pixel_grid(Y, H) + fly;
    const float gx1 = gx + 1.0f, gy1 = gy + 1.0f;
    const float sx = gx1 * sx_scale, sy = gy1 * sy_scale;
    const float fx0 = floorf(sx), fy0 = floorf(sy);
    IsrWarpTaps t;
    t.ix0 = (int)fminf(fmaxf(fx0, -2.f), (float)W); t.iy0 = (int)fminf(fmaxf(fy0, -2.f), (float)H);
    const float wx1 = sx - fx0, wy1 = sy - fy0;
    const float wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    t.vx0 = (unsigned)t.ix0 < (unsigned)W; t.vx1 = (unsigned)(t.ix0 + 1) < (unsigned)W;
    t.vy0 = (unsigned)t.iy0 < (unsigned)H; t.vy1 = (unsigned)(t.iy0 + 1) < (unsigned)H;
    t.w00 = wx0 * wy0; t.w01 = wx1 * wy0; t.w10 = wx0 * wy1; t.w11 = wx1 * wy1;
    t.b00 = (long long)t.iy0 * W + t.ix0;
    return t;
}
