// Small-Cout 3x3 convolution on 4x4x1 MFMA blocks (gfx950, fp32, exact), with the frame-finishing forms of the network's last layer.
//
// The last layer of EnhanceNet maps 64 -> 6 channels (enhancenet.py:124).  On the 32-row MFMA tile
// that wastes 26/32 of the matrix pipe.  v_mfma_f32_4x4x1_16B_f32 instead multiplies sixteen
// independent (4 x 1) x (1 x 4) blocks: with A = the weights of 4 output channels (the same in every
// block: lane l holds channel l % 4) and B = 64 consecutive pixels of one input row (lane l = pixel l),
// one instruction is D[ch][pixel] += w[ch] * x[pixel] for 4 channels x 64 pixels -- the conv's
// natural layout, no padding beyond 6 -> 8 channels, and the result registers are already
// [channel][64 contiguous pixels].  Same rate as every other f32 MFMA (512 flops / 8 cycles).
//
// Workgroup = 4 waves = 16 x 64 output pixels, wave w owns rows 4w..4w+3 and both channel groups
// (8 accumulators of 4 registers).  Input: 4-channel chunks of the haloed 18 x 66 patch, double
// buffered in LDS, the B operand is a plain ds_read_b32 of 64 consecutive floats (row rr, column
// lane + dx); each of those registers feeds every (dy, r) with dy + r = rr and both channel groups
// (2..6 MFMAs).  A operands: per input channel 18 values per lane, kept in LDS as
// [chunk][c][lane % 4][(dx, dy, group)] and read with ds_read_b128 (4 distinct addresses per wave).
// Same fused epilogue semantics as the big kernel (sr_conv3x3.hip: bias, activation, residual).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_conv_common.h"

namespace {

constexpr int SMALL_COUT_VARIANT = 6;          // what conv3x3_small_cout_kernel is recorded as (isrProfileGet)

constexpr int SM_TH = 16, SM_TW = 64;          // output tile
constexpr int SM_PH = SM_TH + 2, SM_PW = SM_TW + 2;
constexpr int SM_CK = 4;                       // input channels per LDS chunk
constexpr int SM_PLANE = SM_PH * SM_PW;        // 1188 floats
constexpr int SM_CHUNK = SM_CK * SM_PLANE;     // 4752
constexpr int SM_NEL = (SM_CHUNK + 255) / 256; // 19 elements per thread and chunk
constexpr int SM_PBUF = SM_NEL * 256;          // 4864: patch buffer, the tail is a sink for masked-off lanes
constexpr int SM_WQ = 20;                      // floats per (c, lane % 4): 18 weights [dx][dy][group] + 2 pad (16-byte rows)
constexpr int SM_WCH = SM_CK * 4 * SM_WQ;      // 320 weight floats per chunk = 80 float4
constexpr int SM_WBUF = 4 * 256;               // every thread writes one float4 (80 real ones)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct SmallConvParams {
    const float* x; const float* wq;           // wq: [chunks][4][4][20], see prepare_weights_small_kernel
    const float* bias8; const float* residual; float* y;
    int N, Cin, H, W, Cout;
    int tilesX, tilesY;
    int act; float slope;
    long long xPlane, xImage;                  // channel / batch strides of x in floats (y and residual are packed)
    int finish;                                // 1: instead of storing y, finish the frame per pixel (fin; N == 1, Cout == 6)
    FinishParams fin;
};

// COLOUR (with p.finish): the frame of a colour network -- three output channels, isr_finish_pixel_colour (isrConvSmallFinishFrameColour)
template <bool COLOUR>
__global__ __launch_bounds__(256, 2) void conv3x3_small_cout_kernel(const SmallConvParams p)
{
    __shared__ __attribute__((aligned(16))) float patch[2][SM_PBUF];
    __shared__ __attribute__((aligned(16))) float wl[2][SM_WBUF];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int tilesPerImage = p.tilesX * p.tilesY;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int n = bid / tilesPerImage;
    const int t = bid - n * tilesPerImage;
    const int ty = t / p.tilesX, tx = t - ty * p.tilesX;
    const int oy0 = ty * SM_TH, ox0 = tx * SM_TW;

    const int planeIn = (int)p.xPlane;
    const float* ximg = p.x + (size_t)n * p.xImage;
    const int nchunks = (p.Cin + SM_CK - 1) / SM_CK;

    unsigned plan[SM_NEL];                     // byte offsets inside a chunk's 4 planes (BAD_OFFSET -> 0)
#pragma unroll
    for (int i = 0; i < SM_NEL; ++i) {
        const int e = tid + i * 256;
        const int c = e / SM_PLANE, rem = e - c * SM_PLANE;
        const int r = rem / SM_PW, col = rem - r * SM_PW;
        const int gy = oy0 + r - 1, gx = ox0 + col - 1;
        const bool ok = e < SM_CHUNK && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        plan[i] = ok ? (unsigned)((c * planeIn + gy * p.W + gx) * 4) : BAD_OFFSET;
    }
    auto chunk_rsrc = [&](int chunk) -> rsrc_t {
        const int left = p.Cin - chunk * SM_CK;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg + (size_t)chunk * SM_CK * planeIn), 0,
                                                 left > 0 ? left * planeIn * 4 : 0, 0x00020000);
    };
    const float4* wq4 = reinterpret_cast<const float4*>(p.wq) + min(tid, SM_WCH / 4 - 1);

    f32x4 acc[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[g][r] = (f32x4){ 0.f, 0.f, 0.f, 0.f };

    {   // prologue: chunk 0
        const rsrc_t rs = chunk_rsrc(0);
        float v[SM_NEL];
        const float4 wv = wq4[0];
#pragma unroll
        for (int i = 0; i < SM_NEL; ++i) v[i] = buf_load(rs, plan[i]);
#pragma unroll
        for (int i = 0; i < SM_NEL; ++i) patch[0][tid + i * 256] = v[i];
        reinterpret_cast<float4*>(wl[0])[tid] = wv;
    }
    __syncthreads();

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < nchunks;
        float sv[SM_NEL];
        float4 wv;
        if (more) {
            const rsrc_t rsn = chunk_rsrc(chunk + 1);
#pragma unroll
            for (int i = 0; i < SM_NEL; ++i) sv[i] = buf_load(rsn, plan[i]);
            wv = wq4[(chunk + 1) * (SM_WCH / 4)];
        }
        __builtin_amdgcn_sched_barrier(0);       // keep the loads above the MFMA block (hipcc would sink them to the stores)
        const float* pw = patch[buf] + (4 * wave) * SM_PW + lane;
        const float* aw = wl[buf] + (lane & 3) * SM_WQ;
#pragma unroll
        for (int c = 0; c < SM_CK; ++c) {
            float a[SM_WQ];
#pragma unroll
            for (int q = 0; q < SM_WQ / 4; ++q) {
                const float4 a4 = *reinterpret_cast<const float4*>(aw + c * 4 * SM_WQ + 4 * q);
                a[4 * q] = a4.x; a[4 * q + 1] = a4.y; a[4 * q + 2] = a4.z; a[4 * q + 3] = a4.w;
            }
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                float b[6];
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) b[rr] = pw[c * SM_PLANE + rr * SM_PW + dx];
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int g = 0; g < 2; ++g)
                            acc[g][r] = __builtin_amdgcn_mfma_f32_4x4x1f32(a[(dx * 3 + dy) * 2 + g], b[dy + r], acc[g][r], 0, 0, 0);
            }
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < SM_NEL; ++i) patch[buf ^ 1][tid + i * 256] = sv[i];
            reinterpret_cast<float4*>(wl[buf ^ 1])[tid] = wv;
        }
        __syncthreads();
    }

    // D register i of group g = channel 4g + i, lane = pixel column
    const int ox = ox0 + lane;
    const size_t plane = (size_t)p.H * p.W;
    if (p.finish) {
        // the frame's last layer: clamp / normalise / shade right here instead of a 50 MB round trip through memory
        // and another launch (isrFinishFrame); the six channels of a pixel sit in this lane's accumulators
        if (ox < p.W) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int oy = oy0 + 4 * wave + r;
                if (oy >= p.H) break;
                if constexpr (COLOUR) {
                    float v[3];
#pragma unroll
                    for (int co = 0; co < 3; ++co) v[co] = acc[0][r][co] + p.bias8[co];
                    isr_finish_pixel_colour(p.fin, ox, oy, v);
                } else {
                    float v[6];
#pragma unroll
                    for (int co = 0; co < 6; ++co) v[co] = acc[co >> 2][r][co & 3] + p.bias8[co];
                    isr_finish_pixel(p.fin, ox, oy, v);
                }
            }
        }
        return;
    }
    if (ox < p.W) {
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = 4 * g + i;
                if (co >= p.Cout) break;
                const float bias = p.bias8[co];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int oy = oy0 + 4 * wave + r;
                    if (oy >= p.H) break;
                    float v = acc[g][r][i] + bias;
                    if (p.act == ISR_ACT_RELU) v = v > 0.f ? v : 0.f;
                    else if (p.act == ISR_ACT_LEAKY) v = v > 0.f ? v : v * p.slope;
                    const size_t o = ((size_t)n * p.Cout + co) * plane + (size_t)oy * p.W + ox;
                    if (p.residual) v += p.residual[o];
                    p.y[o] = v;
                }
            }
    }
}

// wq[chunk][c][q][k]: k = (dx*3 + dy)*2 + g < 18 -> w[4g + q][chunk*4 + c][dy][dx], zero padded
__global__ void prepare_weights_small_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ wq,
                                             float* __restrict__ bias8, int Cout, int Cin)
{
    const int nchunks = (Cin + SM_CK - 1) / SM_CK;
    const int total = nchunks * SM_WCH;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int chunk = e / SM_WCH, rem = e - chunk * SM_WCH;
        const int c = rem / (4 * SM_WQ), q = (rem / SM_WQ) & 3, k = rem % SM_WQ;
        const int dx = k / 6, dy = (k % 6) >> 1, g = k & 1;
        const int co = 4 * g + q, ci = chunk * SM_CK + c;
        wq[e] = (k < 18 && co < Cout && ci < Cin) ? w[((co * Cin + ci) * 3 + dy) * 3 + dx] : 0.f;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) bias8[threadIdx.x] = (bias && (int)threadIdx.x < Cout) ? bias[threadIdx.x] : 0.f;
}

}  // namespace

extern "C" {

int isrConvSmallCinPad(int Cin) { return ((Cin + 7) / 8) * 8; }

long long isrConvSmallWeightFloats(int Cin) { return (long long)((Cin + SM_CK - 1) / SM_CK) * SM_WCH; }

int isrConvSmallPrepare(const float* w, const float* bias, float* w8, float* bias8, int Cout, int Cin, void* stream)
{
    if (!w || !w8 || !bias8 || Cout <= 0 || Cout > 8 || Cin <= 0) return -1;
    const int total = (int)isrConvSmallWeightFloats(Cin);
    hipLaunchKernelGGL(prepare_weights_small_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, bias, w8, bias8, Cout, Cin);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int isrConv3x3SmallCout(const float* x, const float* w8, const float* bias8, const float* residual, float* y,
                        int N, int Cin, int H, int W, int Cout, int act, float slope, void* stream)
{
    return isrConv3x3SmallCoutStrided(x, w8, bias8, residual, y, N, Cin, H, W, Cout, act, slope,
                                      (long long)H * W, (long long)Cin * H * W, stream);
}

int isrConv3x3SmallCoutStrided(const float* x, const float* w8, const float* bias8, const float* residual, float* y,
                               int N, int Cin, int H, int W, int Cout, int act, float slope,
                               long long xPlane, long long xImage, void* stream)
{
    if (!x || !w8 || !bias8 || !y || N <= 0 || Cin <= 0 || Cout <= 0 || Cout > 8 || H <= 0 || W <= 0) return -1;
    if (xPlane < (long long)H * W || (long long)Cin * xPlane * 4 >= (1LL << 31)) return -1;
    if (act < ISR_ACT_NONE || act > ISR_ACT_LEAKY) return -1;
    SmallConvParams p;
    p.x = x; p.wq = w8; p.bias8 = bias8; p.residual = residual; p.y = y;
    p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.tilesX = (W + SM_TW - 1) / SM_TW; p.tilesY = (H + SM_TH - 1) / SM_TH;
    p.act = act; p.slope = slope;
    p.xPlane = xPlane; p.xImage = xImage;
    p.finish = 0;
    const long long nwg = (long long)N * p.tilesX * p.tilesY;
    if (nwg > 0x7fffffffLL) return -1;
    return isr_launch(SMALL_COUT_VARIANT, 2.0 * 9 * Cin * Cout * (double)N * H * W, conv3x3_small_cout_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream, p);
}

int isrConvSmallFinishFrame(const float* x, const float* w8, const float* bias8, const float* net_input, float* next_prev, float* rgb,
                            int Cin, int h, int w, long long xPlane, const float* shading24, int exponent, float ao_strength,
                            int inverse_ao, int enable_specular, void* stream)
{
    if (!x || !w8 || !bias8 || !net_input || !next_prev || Cin <= 0 || h <= 0 || w <= 0 || (rgb && !shading24)) return -1;
    const int H = 4 * h, W = 4 * w;
    if (xPlane < (long long)H * W || (long long)Cin * xPlane * 4 >= (1LL << 31)) return -1;
    SmallConvParams p;
    p.x = x; p.wq = w8; p.bias8 = bias8; p.residual = nullptr; p.y = nullptr;
    p.N = 1; p.Cin = Cin; p.H = H; p.W = W; p.Cout = 6;
    p.tilesX = (W + SM_TW - 1) / SM_TW; p.tilesY = (H + SM_TH - 1) / SM_TH;
    p.act = ISR_ACT_NONE; p.slope = 0.f;
    p.xPlane = xPlane; p.xImage = (long long)Cin * xPlane;
    p.finish = 1;
    isr_fill_finish_params(p.fin, nullptr, net_input, next_prev, rgb, h, w, shading24, exponent, ao_strength, inverse_ao, enable_specular);
    return isr_launch(SMALL_COUT_VARIANT, 2.0 * 9 * Cin * 6 * (double)H * W, conv3x3_small_cout_kernel<false>, dim3((unsigned)(p.tilesX * p.tilesY)), dim3(256), 0, (hipStream_t)stream, p);
}

int isrConvSmallFinishFrameColour(const float* x, const float* w8, const float* bias8, const float* net_input, float* out3,
                                  int Cin, int h, int w, long long xPlane, void* stream)
{
    if (!x || !w8 || !bias8 || !net_input || !out3 || Cin <= 0 || h <= 0 || w <= 0) return -1;
    const int H = 4 * h, W = 4 * w;
    if (xPlane < (long long)H * W || (long long)Cin * xPlane * 4 >= (1LL << 31)) return -1;
    SmallConvParams p;
    p.x = x; p.wq = w8; p.bias8 = bias8; p.residual = nullptr; p.y = nullptr;
    p.N = 1; p.Cin = Cin; p.H = H; p.W = W; p.Cout = 3;
    p.tilesX = (W + SM_TW - 1) / SM_TW; p.tilesY = (H + SM_TH - 1) / SM_TH;
    p.act = ISR_ACT_NONE; p.slope = 0.f;
    p.xPlane = xPlane; p.xImage = (long long)Cin * xPlane;
    p.finish = 1;
    isr_fill_finish_params(p.fin, nullptr, net_input, out3, nullptr, h, w, nullptr, 1, 0.f, 0, 0);
    return isr_launch(SMALL_COUT_VARIANT, 2.0 * 9 * Cin * 3 * (double)H * W, conv3x3_small_cout_kernel<true>, dim3((unsigned)(p.tilesX * p.tilesY)), dim3(256), 0, (hipStream_t)stream, p);
}

}  // extern "C"
