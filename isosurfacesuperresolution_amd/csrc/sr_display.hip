// The display stage of the viewer's frame (include/isr_sr_kernels.h: isrDisplayFrame): everything the reference viewer does between the
// network and the window (SuperresolutionNetwork/mainGUI.py:603-608,626-636,762-853) in ONE launch, one thread per high-resolution pixel.
//
// DEFINED operation by operation in isosurfacesuperresolution_amd/viewer.py: compose_display (elementwise fp32 torch operations, one IEEE
// rounding each) and computed here with the same operations in the same order and no contraction into FMAs (`#pragma clang fp
// contract(off)` in every function that takes part): wherever no shading enters, the same bits.  The focus window's shading is the
// arithmetic of isr_finish_pixel (sr_finish.h) restated -- that function also reconstructs and stores the frame, and is left as it is --
// and agrees with utils.ScreenSpaceShading to 1e-4, as isrFinishFrame does.
//
// A thread computes only the channels its view shows (of the reference's twelve, the views read 0:3, 3, 4:7, 7 and 10).  Plain global
// stores, no LDS, no communication between threads.
//
// isrDisplayBaselineFrame is the same frame in the viewer's non-network render modes (mainGUI.py:712-757; viewer.py: compose_baseline):
// the image is the rendered G-buffer, shaded at ITS resolution and interpolated x4 with all its channels (nearest, bilinear, bicubic), or
// the full-resolution G-buffer as it is (ground truth).  Focus blend, channel view, post-smoothing and the stores are the device functions
// of display_frame_kernel, shared.  Interpolated modes: a pre-pass over the h x w low-resolution pixels writes the planes the view shows
// (colour: shaded once per low pixel, not once per tap), the display launch reads them with coalesced loads -- profiles/render_modes.md.
#include <hip/hip_runtime.h>
#include "../../include/isr_sr_kernels.h"
#include "sr_warp_exact.h"

namespace {

// the x4 bilinear taps of a high-resolution pixel (models/videotools.py: VideoTools.upscale_bilinear)
struct UpTaps { int y0, y1, x0, x1; float hy, hx, ly, lx; };

// channel c of the low-resolution G-buffer as the viewer holds it: the mask channel mapped to [-1, +1] (mainGUI.py:714-717)
__device__ __forceinline__ float low_value(const float* g, int w, int y, int x, int c)
{
#pragma clang fp contract(off)
    const float v = g[((size_t)y * w + x) * 12 + c];
    if (c != 3) return v;
    const float twice = v * 2.0f;
    return twice - 1.0f;
}

__device__ __forceinline__ float low_upscaled(const IsrDisplayParams& p, const UpTaps& t, int c)
{
#pragma clang fp contract(off)
    return isr_bilerp_rn(t.hy, t.hx, t.ly, t.lx, low_value(p.gbuffer, p.w, t.y0, t.x0, c), low_value(p.gbuffer, p.w, t.y0, t.x1, c),
                         low_value(p.gbuffer, p.w, t.y1, t.x0, c), low_value(p.gbuffer, p.w, t.y1, t.x1, c));
}

// channel c of the twelve-channel image before masking and focus (mainGUI.py:603-608 unshaded, :626-628 colour networks)
__device__ __forceinline__ float base_channel(const IsrDisplayParams& p, const UpTaps& t, int c, size_t pix, size_t hplane)
{
    if (c < 3) return p.rgb[(size_t)c * hplane + pix];
    if (p.raw) {
        if (c <= 7) return p.raw[(size_t)(c - 3) * hplane + pix];
        if (c == 10) return p.raw[5 * hplane + pix];
    }
    return low_upscaled(p, t, c);
}

// clamp(ScreenSpaceShading(mask, normal, ., ao), 0, 1) of one full-resolution pixel (utils/shading.py; the lines of isr_finish_pixel)
template <class P>
__device__ __forceinline__ void shade_pixel(const P& p, float mask, float nx, float ny, float nz, float ao, float (&col)[3])
{
#pragma clang fp contract(off)
    const float* ambient = p.shading, * diffuse = p.shading + 3, * specular = p.shading + 6, * light = p.shading + 9,
               * material = p.shading + 12, * background = p.shading + 15;
    const float aof = p.ao_strength * fminf(fmaxf(ao, 0.f), 1.f) + (1.0f - p.ao_strength);
    const float ndl = light[0] * nx + light[1] * ny + light[2] * nz;
    float spec = 0.f;
    if (p.enable_specular) {
        const float rz = 2.f * ndl * nz - light[2];            // eye direction is (0,0,1) everywhere
        const float base = fminf(fmaxf(rz, 0.f), 1.f);
        float pw = 1.f;
        for (int e = 0; e < p.exponent; ++e) pw *= base;
        spec = ((float)(p.exponent + 2) / (2.0f * 3.14159265358979323846f)) * pw;
    }
    const float t = fminf(fmaxf(mask * 0.5f + 0.5f, 0.f), 1.f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float c = ambient[k] * material[k] + (diffuse[k] * material[k]) * fabsf(ndl) + spec * specular[k];
        c *= aof;
        c = background[k] + t * (c - background[k]);
        col[k] = fminf(fmaxf(c, 0.f), 1.f);
    }
}

__device__ __forceinline__ unsigned to_byte(float v)
{
#pragma clang fp contract(off)
    const float c = fminf(fmaxf(v, 0.f), 1.f);
    return (unsigned)rintf(c * 255.0f);           // round half to even, as torch.round
}

// the channels of the twelve a view reads: c0 .. c0 + n - 1 (the flow view reads none)
__device__ __forceinline__ void view_channels(int channel, int& c0, int& n)
{
    c0 = 0; n = 3;
    switch (channel) {
    case ISR_VIEW_MASK:   c0 = 3;  n = 1; break;
    case ISR_VIEW_NORMAL: c0 = 4;  n = 3; break;
    case ISR_VIEW_DEPTH:  c0 = 7;  n = 1; break;
    case ISR_VIEW_AO:     c0 = 10; n = 1; break;
    default: break;
    }
}

// upscale_bilinear(cat(flow, 0) * 10 + 0.5)   (mainGUI.py:818-825, with the frame's own hole-filled flow)
__device__ __forceinline__ void flow_view(const float* flow, int w, size_t lplane, const UpTaps& t, float (&out)[3])
{
#pragma clang fp contract(off)
    const int i00 = t.y0 * w + t.x0, i01 = t.y0 * w + t.x1, i10 = t.y1 * w + t.x0, i11 = t.y1 * w + t.x1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float* q = flow + (size_t)k * lplane;
        const float a = q[i00] * 10.0f, b = q[i01] * 10.0f, c = q[i10] * 10.0f, d = q[i11] * 10.0f;
        out[k] = isr_bilerp_rn(t.hy, t.hx, t.ly, t.lx, a + 0.5f, b + 0.5f, c + 0.5f, d + 0.5f);
    }
    out[2] = isr_bilerp_rn(t.hy, t.hx, t.ly, t.lx, 0.5f, 0.5f, 0.5f, 0.5f);
}

// image = m foc + (1 - m) image where m > 0 inside the viewport; the full-resolution G-buffer is read here only (mainGUI.py:787-798)
template <class P>
__device__ __forceinline__ void focus_blend(const P& p, int X, int Y, size_t pix, int c0, int n, float (&v)[3])
{
#pragma clang fp contract(off)
    if (p.focus && X >= p.viewport[0] && Y >= p.viewport[1] && X < p.viewport[2] && Y < p.viewport[3]) {
        const float m = p.focus_mask[pix];
        if (m > 0.f) {
            const float* f = p.focus + pix * 12;
            const float fmask2 = f[3] * 2.0f;
            const float fmask = fmask2 - 1.0f;
            float fv[3] = { 0.f, 0.f, 0.f };
            if (c0 == 0) {
                shade_pixel(p, fmask, f[4], f[5], f[6], f[10], fv);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < n) fv[k] = (c0 + k == 3) ? fmask : f[c0 + k];
            }
            const float om = 1.0f - m;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float a = m * fv[k], b = om * v[k];
                v[k] = a + b;
            }
        }
    }
}

// the channel view of the image's channels v (mainGUI.py:803-828)
__device__ __forceinline__ void view_output(int channel, const float* depth_bounds, const float (&v)[3], float (&out)[3])
{
#pragma clang fp contract(off)
    switch (channel) {
    case ISR_VIEW_MASK: case ISR_VIEW_AO:
        out[0] = out[1] = out[2] = v[0];
        break;
    case ISR_VIEW_NORMAL:
#pragma unroll
        for (int k = 0; k < 3; ++k) { const float s = v[k] * 0.5f; out[k] = s + 0.5f; }
        break;
    case ISR_VIEW_DEPTH: {
        const float lo = depth_bounds[0], hi = depth_bounds[1];
        const float num = v[0] - lo, den = hi - lo;
        out[0] = out[1] = out[2] = num / den;
        break;
    }
    default:
        out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
        break;
    }
}

// smooth_prev * warp_upscale(previous displayed, flow, 4) + smooth_cur * image (mainGUI.py:835-849), then the stores: fp32 planes, RGBA
template <class P>
__device__ __forceinline__ void smooth_and_store(const P& p, int X, int Y, size_t pix, size_t hplane, size_t lplane, float (&out)[3])
{
#pragma clang fp contract(off)
    const int W = 4 * p.w;
    if (p.prev) {
        const IsrWarpTaps wt = isr_warp_taps(p.flow, p.flow + lplane, p.h, p.w, X, Y);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* q = p.prev + (size_t)c * hplane;
            float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f;
            if (wt.vy0 && wt.vx0) v00 = q[wt.b00];
            if (wt.vy0 && wt.vx1) v01 = q[wt.b00 + 1];
            if (wt.vy1 && wt.vx0) v10 = q[wt.b00 + W];
            if (wt.vy1 && wt.vx1) v11 = q[wt.b00 + W + 1];
            // ((v00 w00 + v01 w01) + v10 w10) + v11 w11, one rounding per operation
            const float t00 = v00 * wt.w00, t01 = v01 * wt.w01, t10 = v10 * wt.w10, t11 = v11 * wt.w11;
            float r = t00 + t01;
            r = r + t10;
            r = r + t11;
            const float a = p.smooth_prev * r, b = p.smooth_cur * out[c];
            out[c] = a + b;
        }
    }

    p.out[pix] = out[0];
    p.out[hplane + pix] = out[1];
    p.out[2 * hplane + pix] = out[2];
    if (p.out8)
        reinterpret_cast<unsigned*>(p.out8)[pix] = to_byte(out[0]) | (to_byte(out[1]) << 8) | (to_byte(out[2]) << 16) | 0xff000000u;
}

__device__ __forceinline__ UpTaps up_taps(int X, int Y, int h, int w)
{
#pragma clang fp contract(off)
    UpTaps t;
    isr_src_index_rn(Y, 0.25f, h, t.y0, t.y1, t.ly);
    isr_src_index_rn(X, 0.25f, w, t.x0, t.x1, t.lx);
    t.hy = 1.f - t.ly; t.hx = 1.f - t.lx;
    return t;
}

__global__ void __launch_bounds__(256) display_frame_kernel(const IsrDisplayParams p)
{
#pragma clang fp contract(off)
    const int H = 4 * p.h, W = 4 * p.w;
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= W || Y >= H) return;
    const size_t hplane = (size_t)H * W, lplane = (size_t)p.h * p.w;
    const size_t pix = (size_t)Y * W + X;
    const UpTaps t = up_taps(X, Y, p.h, p.w);

    float out[3];
    if (p.channel == ISR_VIEW_FLOW) {
        flow_view(p.flow, p.w, lplane, t, out);
    } else {
        int c0, n;
        view_channels(p.channel, c0, n);
        float v[3] = { 0.f, 0.f, 0.f };
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n) v[k] = base_channel(p, t, c0 + k, pix, hplane);
        if (p.masking) {
            // image = bg + (base_mask / 2 + 1 / 2) (image - bg), base_mask the UPSCALED low-resolution mask (mainGUI.py:630-636)
            const float half = low_upscaled(p, t, 3) * 0.5f;
            const float tm = half + 0.5f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float d = v[k] - p.background0;
                const float s = tm * d;
                v[k] = p.background0 + s;
            }
        }
        focus_blend(p, X, Y, pix, c0, n, v);
        view_output(p.channel, p.depth_bounds, v, out);
    }
    smooth_and_store(p, X, Y, pix, hplane, lplane, out);
}

// ---- the non-network render modes ------------------------------------------------------------------------------------------------------
// The pre-pass of the interpolated modes, one thread per LOW-resolution pixel: the planes c0 .. c0 + n - 1 of the viewer's twelve-channel
// low image (mainGUI.py:712-720) -- mask mapped to [-1, +1], colour = clamp(shading(mask, normal, ., ao), 0, 1) -- written planar.
__global__ void __launch_bounds__(256) baseline_low_kernel(const IsrDisplayBaselineParams p)
{
#pragma clang fp contract(off)
    const size_t lplane = (size_t)p.h * p.w;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= lplane) return;
    const float* g = p.gbuffer + i * 12;
    int c0, n;
    view_channels(p.channel, c0, n);
    float v[3] = { 0.f, 0.f, 0.f };
    if (c0 == 0) {
        const float twice = g[3] * 2.0f;
        shade_pixel(p, twice - 1.0f, g[4], g[5], g[6], g[10], v);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < n) {
                const float twice = g[c0 + k] * 2.0f;
                v[k] = (c0 + k == 3) ? twice - 1.0f : g[c0 + k];
            }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (k < n) p.low_planes[(size_t)(c0 + k) * lplane + i] = v[k];
}

// The x4 bicubic taps of one axis (models/videotools.py: upscale_bicubic; ATen's upsample_bicubic2d with A = -0.75, align_corners=False):
// src = 0.25 (dst + 0.5) - 0.5, i = floor(src), t = src - i in { 0.625, 0.875, 0.125, 0.375 } for dst % 4 = 0 .. 3; taps i - 1 .. i + 2
// clamped to the image, weights c2(t + 1), c1(t), c1(1 - t), c2(2 - t) -- all sixteen exact in fp32.
__device__ const float BICUBIC_X4[4][4] = {
    { -0.06591796875f, 0.42626953125f, 0.74951171875f, -0.10986328125f },
    { -0.01025390625f, 0.11474609375f, 0.96728515625f, -0.07177734375f },
    { -0.07177734375f, 0.96728515625f, 0.11474609375f, -0.01025390625f },
    { -0.10986328125f, 0.74951171875f, 0.42626953125f, -0.06591796875f } };

__device__ __forceinline__ void bicubic_taps(int dst, int n, int (&idx)[4])
{
    const int i = (dst >> 2) - ((dst & 3) < 2 ? 1 : 0);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(i - 1 + k, 0), n - 1);
}

// ((w0 v0 + w1 v1) + w2 v2) + w3 v3, one rounding per operation
__device__ __forceinline__ float cubic_sum(const float* w, float v0, float v1, float v2, float v3)
{
#pragma clang fp contract(off)
    const float t0 = w[0] * v0, t1 = w[1] * v1, t2 = w[2] * v2, t3 = w[3] * v3;
    float r = t0 + t1;
    r = r + t2;
    r = r + t3;
    return r;
}

__global__ void __launch_bounds__(256) display_baseline_kernel(const IsrDisplayBaselineParams p)
{
#pragma clang fp contract(off)
    const int H = 4 * p.h, W = 4 * p.w;
    const int X = blockIdx.x * 256 + threadIdx.x, Y = blockIdx.y;
    if (X >= W || Y >= H) return;
    const size_t hplane = (size_t)H * W, lplane = (size_t)p.h * p.w;
    const size_t pix = (size_t)Y * W + X;

    float out[3];
    if (p.channel == ISR_VIEW_FLOW) {
        flow_view(p.flow, p.w, lplane, up_taps(X, Y, p.h, p.w), out);
    } else {
        int c0, n;
        view_channels(p.channel, c0, n);
        float v[3] = { 0.f, 0.f, 0.f };
        if (p.mode == ISR_BASE_IDENTITY) {
            const float* g = p.gbuffer + pix * 12;
            const float twice = g[3] * 2.0f;
            const float mask = twice - 1.0f;
            if (c0 == 0) {
                shade_pixel(p, mask, g[4], g[5], g[6], g[10], v);
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < n) v[k] = (c0 + k == 3) ? mask : g[c0 + k];
            }
        } else if (p.mode == ISR_BASE_NEAREST) {
            const size_t src = (size_t)(Y >> 2) * p.w + (X >> 2);
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < n) v[k] = p.low_planes[(size_t)(c0 + k) * lplane + src];
        } else if (p.mode == ISR_BASE_BILINEAR) {
            const UpTaps t = up_taps(X, Y, p.h, p.w);
            const int i00 = t.y0 * p.w + t.x0, i01 = t.y0 * p.w + t.x1, i10 = t.y1 * p.w + t.x0, i11 = t.y1 * p.w + t.x1;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < n) {
                    const float* q = p.low_planes + (size_t)(c0 + k) * lplane;
                    v[k] = isr_bilerp_rn(t.hy, t.hx, t.ly, t.lx, q[i00], q[i01], q[i10], q[i11]);
                }
        } else {
            int xs[4], ys[4];
            bicubic_taps(X, p.w, xs);
            bicubic_taps(Y, p.h, ys);
            const float* wx = BICUBIC_X4[X & 3], * wy = BICUBIC_X4[Y & 3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (k < n) {
                    const float* q = p.low_planes + (size_t)(c0 + k) * lplane;
                    float rows[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {                   // the horizontal pass first, then the vertical one over its four results
                        const float* r = q + (size_t)ys[j] * p.w;
                        rows[j] = cubic_sum(wx, r[xs[0]], r[xs[1]], r[xs[2]], r[xs[3]]);
                    }
                    v[k] = cubic_sum(wy, rows[0], rows[1], rows[2], rows[3]);
                }
        }
        focus_blend(p, X, Y, pix, c0, n, v);
        view_output(p.channel, p.depth_bounds, v, out);
    }
    smooth_and_store(p, X, Y, pix, hplane, lplane, out);
}

}  // namespace

extern "C" {

int isrDisplayFrame(const IsrDisplayParams* params, void* stream)
{
    if (!params) return -1;
    const IsrDisplayParams& p = *params;
    if (!p.gbuffer || !p.rgb || !p.out || p.h <= 0 || p.w <= 0) return -1;
    if (p.h > 16383 || p.w > 16383) return -1;                                   // (4 h is a grid dimension; h w indexes in int)
    if (p.channel < ISR_VIEW_COLOR || p.channel > ISR_VIEW_FLOW) return -1;
    if ((p.channel == ISR_VIEW_FLOW || p.prev) && !p.flow) return -1;
    if (p.channel == ISR_VIEW_DEPTH && !p.depth_bounds) return -1;
    if (p.focus && !p.focus_mask) return -1;
    if (p.prev == p.out) return -1;                                              // the warp reads neighbouring pixels
    if (p.out8 && ((size_t)p.out8 & 3)) return -1;
    if (p.exponent < 0) return -1;
    hipLaunchKernelGGL(display_frame_kernel, dim3((4 * p.w + 255) / 256, 4 * p.h), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int isrDisplayBaselineFrame(const IsrDisplayBaselineParams* params, void* stream)
{
    if (!params) return -1;
    const IsrDisplayBaselineParams& p = *params;
    if (!p.gbuffer || !p.out || p.h <= 0 || p.w <= 0) return -1;
    if (p.h > 16383 || p.w > 16383) return -1;
    if (p.mode < ISR_BASE_NEAREST || p.mode > ISR_BASE_IDENTITY) return -1;
    if (p.channel < ISR_VIEW_COLOR || p.channel > ISR_VIEW_FLOW) return -1;
    const bool identity = p.mode == ISR_BASE_IDENTITY;
    if (identity && (p.prev || p.focus || p.channel == ISR_VIEW_FLOW)) return -1;
    const bool planes = !identity && p.channel != ISR_VIEW_FLOW;
    if (planes && !p.low_planes) return -1;
    if ((p.channel == ISR_VIEW_FLOW || p.prev) && !p.flow) return -1;
    if (p.channel == ISR_VIEW_DEPTH && !p.depth_bounds) return -1;
    if (p.focus && !p.focus_mask) return -1;
    if (p.prev == p.out) return -1;
    if (p.out8 && ((size_t)p.out8 & 3)) return -1;
    if (p.exponent < 0) return -1;
    if (planes) {
        const size_t lplane = (size_t)p.h * p.w;
        hipLaunchKernelGGL(baseline_low_kernel, dim3((unsigned)((lplane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    }
    hipLaunchKernelGGL(display_baseline_kernel, dim3((4 * p.w + 255) / 256, 4 * p.h), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
