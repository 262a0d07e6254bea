// The three pieces of the RCAN generator (models/rcan.py) that are not convolutions (include/isr_sr_kernels.h: isrChannelPool,
// isrChannelGateScaleAdd, isrShuffleTailColour).  All three are memory bound: 16-byte accesses wherever base address and strides allow
// them, a per-element path otherwise; no floating-point atomics; plain pointer stores.
//
//   channel attention of one residual block, y = x + t * s[c], s = sigmoid(Wu leaky(Wd mean_hw(t) + bd) + bu), in TWO launches:
//     channel_pool_kernel      slab sums of every plane of t in fp64 -> workspace double [N][64][S]
//     gate_scale_add_kernel    every workgroup: the S partials of its image summed in index order, the fp32 mean z[64], the 64 -> 4 -> 64
//                              perceptron (recomputed per workgroup: 512 multiply-adds), then its share of one plane of y
//   the network's tail, out = conv3x3(pixel_shuffle(f, 4), w [Cout][4][3][3]) + b, in ONE launch:
//     shuffle_tail_kernel      the low-resolution tile and its one-pixel halo are staged in LDS already shuffled; the four-channel
//                              high-resolution tensor never exists in memory
//
// TRAINING (include/isr_sr_kernels.h: isrChannelGateGradSums, isrChannelGateScaleBackward, isrChannelGateParamGrad,
// isrShuffleTailDataGrad, isrShuffleTailWeightGrad).  Given dy, the attention's dx IS dy (no launch); the rest of a block's backward is
// at most THREE launches:
//     gate_grad_sum_kernel     slab sums of dy * t in fp64 -> workspace double [N][64][S] (channel_pool_kernel's slabs and alignment classes)
//     gate_backward_kernel     every workgroup: ds[64] of its image from the S partials, the perceptron's backward (recomputed per
//                              workgroup from the saved mean z and gate s: 768 multiply-adds), then its share of one plane of
//                              dt = dy * s + dz[c] / (H W)
//     gate_param_grad_kernel   ONE workgroup, its own tiny launch (not a designated workgroup of the streaming launch: that one is
//                              skipped when t needs no gradient, and its workgroups have no order): dWu, dbu, dWd, dbd summed over the
//                              images in index order
//   and the tail's backward three:
//     shuffle_tail_dgrad_kernel      the dout tile (32 x 64 and a one-pixel halo, four output channels at a time) staged in LDS; a thread
//                                    owns one low-resolution pixel and two of the four channels of P: 2 x 16 chains, stored un-shuffled
//                                    as df[16 ci + 4 i + j][y][x]; the four-channel high-resolution gradient never exists in memory
//     shuffle_tail_wgrad_kernel      P restaged from f as in the forward; per tile and output channel the 36 weight terms and the bias
//                                    term in fp64 -> workspace double [tiles][Cout][37]
//     shuffle_tail_wgrad_sum_kernel  the tiles' partials summed in index order, rounded to fp32 once
//
// ORDER OF THE ARITHMETIC (what the tests' bounds are derived from; nothing below is contracted or reassociated by the compiler:
// file-scope pragma, explicit fmaf):
//   pool   : a thread adds its elements in index order in fp64, the workgroup's 256 sums go through an LDS tree of fixed shape: a result
//            depends on the shape, the slab count and the alignment class of the tensor only -- two runs give the same bits.
//   mean   : sum = ((p[0] + p[1]) + ...) + p[S - 1] in fp64; z = (float)(sum / (double)(H W)).
//   gate   : a[j] = bd[j], then a[j] = fmaf(Wd[j][c], z[c], a[j]) for c = 0 .. 63; g[j] = a[j] > 0 ? a[j] : a[j] * slope;
//            u = bu[c], then u = fmaf(Wu[c][j], g[j], u) for j = 0 .. 3; s = 1 / (1 + expf(-u)).
//   y      : m = t * s, y = x + m as two separately rounded operations (scale_add below): the two roundings of `x + t * s` in PyTorch.
//            (NOT __fadd_rn(x, __fmul_rn(t, s)): HIP's header defines those two as plain operators compiled under hipcc's default
//            -ffp-contract=fast, and once inlined the pair is fused into one v_fma_f32; operators written below the pragma are not.)
//   tail   : acc = b[co], then acc = fmaf(w[co][ci][ky][kx], P[ci][Y + ky - 1][X + kx - 1], acc) for ci, ky, kx in this nesting, P = 0
//            outside the image; P[ci][4 y + i][4 x + j] = f[16 ci + 4 i + j][y][x].  A pixel's chain does not depend on the tile it is in.
//   ds     : m = dy * t rounded to fp32, then exactly pool's order with m in the place of t; ds[c] = (float)(((p[0] + p[1]) + ...) + p[S - 1]).
//   gate'  : du[c] = ds[c] * (s[c] * (1 - s[c])) (three roundings, s the gate the forward stored); a[j], g[j] as in `gate` from the saved z;
//            dg[j] = (float)(fp64 sum over c = 0 .. 63 in index order of the exact products Wu[c][j] du[c]); da[j] = a[j] > 0 ? dg[j] : dg[j] * slope;
//            dz[c] = 0, then dz[c] = fmaf(Wd[j][c], da[j], dz[c]) for j = 0 .. 3; q[c] = (float)((double)dz[c] / (double)(H W)).
//   dt     : m = dy * s, dt = q + m as two separately rounded operations (scale_add): with Wu = 0 the bits of dy * s.
//   params : per entry an fp64 sum over n = 0 .. N - 1 in index order of the (exact) fp64 products du[n][c] g[n][j] (dWu), da[n][j] z[n][c]
//            (dWd) or of du[n][c] (dbu), da[n][j] (dbd), rounded to fp32 once.
//   dgrad  : dP = 0, then dP = fmaf(w[co][ci][2 - ky][2 - kx], dout[co][Y + ky - 1][X + kx - 1], dP) for co, ky, kx in this nesting, dout = 0
//            outside the image; df[16 ci + 4 i + j][y][x] = dP[ci][4 y + i][4 x + j].  A value's chain does not depend on the tile it is in.
//   wgrad  : a thread owns the pixels (Y, 4 qx .. 4 qx + 3) of rows Y = ry and ry + 16 of its tile and adds, in fp64, in this order: rows,
//            then terms (ci, ky, kx), then the four pixels -- each product of two fp32 values is exact in fp64; the bias term adds the four
//            dout of a row before the weight terms.  The 64 lanes of a wave are summed by a butterfly (lane ^ 1, 2, 4, 8, 16, 32), the four
//            waves in index order, the tiles ((n, tile row, tile column) order) in index order; one rounding to fp32 at the end.
#include "sr_split_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AT_C = 64;               // channels
constexpr int AT_R = 4;                // reduced channels of the attention's perceptron
constexpr int AT_THREADS = 256;
constexpr int AT_MAX_SLABS = 64;
constexpr int AT_SLAB_PIXELS = 4096;   // a slab is at least this long (except the only one)
constexpr int AT_POOL_GROUPS = 1024;   // N * 64 * S aims at this many workgroups (four per CU)
constexpr int AT_CHUNK = 8192;         // elements of one plane a gate_scale_add workgroup handles: 1024 workgroups at 480 x 270
constexpr int ISR_VARIANT_CHANNEL_POOL = 39;    // ops.VARIANT_NAMES
constexpr int ISR_VARIANT_GATE_SCALE_ADD = 40;
constexpr int ISR_VARIANT_SHUFFLE_TAIL = 41;
constexpr int ISR_VARIANT_GATE_GRAD_SUM = 42;
constexpr int ISR_VARIANT_GATE_BACKWARD = 43;
constexpr int ISR_VARIANT_GATE_PARAM_GRAD = 44;
constexpr int ISR_VARIANT_SHUFFLE_TAIL_DGRAD = 45;
constexpr int ISR_VARIANT_SHUFFLE_TAIL_WGRAD = 46;
constexpr int ISR_VARIANT_SHUFFLE_TAIL_WGRAD_SUM = 47;

constexpr int TL_H = 8, TL_W = 16;                       // low-resolution tile of the shuffle tail
constexpr int TP_H = TL_H + 2, TP_W = TL_W + 2;          // ... with its halo
constexpr int TS_H = 4 * TP_H, TS_W = 4 * TP_W;          // the shuffled patch: 40 x 72 per channel
constexpr int TS_STRIDE = TS_W + 4;                      // ... rows 76 floats apart: the 16-byte staging path then writes LDS without bank
                                                         // conflicts (a wave's 64 lanes: 4 j x 4 quads x 4 i -> banks j + 16 q + 12 i + 4 k, all different)
constexpr int TAIL_MAX_COUT = 8;
constexpr int TD_CO = 4;                                 // output channels of dout the data gradient stages at a time
constexpr int TD_H = 4 * TL_H + 2, TD_W = 4 * TL_W + 2;  // the dout tile with its halo: 34 x 66 per channel
constexpr int TD_STRIDE = TD_W + 2;                      // ... rows 68 floats apart: a thread's six columns start at a multiple of 16 bytes
constexpr int TW_TERMS = 37;                             // per output channel: 36 weight terms [ci][ky][kx] and the bias term
constexpr int TW_MAX_TILES = 1 << 20;

// x + t * s with the product rounded before the sum (never one fused multiply-add: contraction is off from the pragma on)
__device__ __forceinline__ float scale_add(float x, float t, float s)
{
    const float m = t * s;
    return x + m;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int pool_slabs(int N, int H, int W)
{
    const long long hw = (long long)H * W;
    long long s = (hw + AT_SLAB_PIXELS - 1) / AT_SLAB_PIXELS;
    const long long most = AT_POOL_GROUPS / ((long long)N * AT_C) > 1 ? AT_POOL_GROUPS / ((long long)N * AT_C) : 1;
    if (s > most) s = most;
    if (s > AT_MAX_SLABS) s = AT_MAX_SLABS;
    if (s < 1) s = 1;
    // slabs are whole 16-byte quads; the count that leaves none of them empty
    const long long chunk = (((hw + s - 1) / s) + 3) / 4 * 4;
    return (int)((hw + chunk - 1) / chunk);
}

long long pool_chunk(long long hw, int S) { return (((hw + S - 1) / S) + 3) / 4 * 4; }

bool attention_supported(int N, int C, int R, int H, int W, long long plane, long long image)
{
    if (N <= 0 || N > 65535 || C != AT_C || R != AT_R || H <= 0 || W <= 0) return false;
    const long long hw = (long long)H * W;
    if (plane < hw || image < (long long)AT_C * plane) return false;
    return image * 4 < (1ll << 31);
}

// the workgroup's 256 fp64 sums through an LDS tree of fixed shape; the total is in sh[0] afterwards
__device__ __forceinline__ void tree_sum(double* sh, double acc, int tid)
{
    sh[tid] = acc;
    __syncthreads();
    for (int k = AT_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) sh[tid] = sh[tid] + sh[tid + k];
        __syncthreads();
    }
}

struct PoolParams {
    const float* t; long long tPlane, tImage;
    long long hw, chunk;
    int S, vec;
    double* ws;
};

__global__ void __launch_bounds__(AT_THREADS) channel_pool_kernel(const PoolParams p)
{
    __shared__ double sh[AT_THREADS];
    const int s = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const float* plane = p.t + (long long)n * p.tImage + (long long)c * p.tPlane;
    const long long lo = (long long)s * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;          // the pad behind H W is never read
    double acc = 0.0;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* q4 = reinterpret_cast<const float4*>(plane + lo);
        for (long long q = tid; q < quads; q += AT_THREADS) {
            const float4 v = q4[q];
            acc = acc + (double)v.x;
            acc = acc + (double)v.y;
            acc = acc + (double)v.z;
            acc = acc + (double)v.w;
        }
        const long long rest = lo + 4 * quads + tid;                         // at most three elements, in the last slab
        if (tid < 3 && rest < hi) acc = acc + (double)plane[rest];
    } else {
        for (long long i = lo + tid; i < hi; i += AT_THREADS) acc = acc + (double)plane[i];
    }
    tree_sum(sh, acc, tid);
    if (tid == 0) p.ws[((long long)n * AT_C + c) * p.S + s] = sh[0];
}

// the fp32 mean of plane (n, c) from its S partial sums, in index order
__device__ __forceinline__ float pooled_mean(const double* ws, int n, int c, int S, long long hw)
{
    const double* q = ws + ((long long)n * AT_C + c) * S;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum = sum + q[s];
    return (float)(sum / (double)hw);
}

__global__ void __launch_bounds__(AT_THREADS) channel_mean_kernel(const double* ws, int S, long long hw, int planes, float* mean)
{
    const int i = blockIdx.x * AT_THREADS + threadIdx.x;
    if (i < planes) mean[i] = pooled_mean(ws, i / AT_C, i % AT_C, S, hw);
}

struct GateParams {
    const float* x; const float* t; float* y;
    long long xPlane, xImage, tPlane, tImage, yPlane, yImage;
    long long hw, chunk;
    const double* ws; int S;
    const float* wd; const float* bd; const float* wu; const float* bu;
    float slope;
    float* gate;                 // [N][64] or NULL
    int vec;
    unsigned* absmax;            // range guard (may be NULL), as SplitConvParams::absmax: over every y stored
};

__global__ void __launch_bounds__(AT_THREADS) gate_scale_add_kernel(const GateParams p)
{
    __shared__ float z[AT_C];
    __shared__ float g[AT_R];
    __shared__ float sgate;
    const int k = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    if (tid < AT_C) z[tid] = pooled_mean(p.ws, n, tid, p.S, p.hw);
    __syncthreads();
    if (tid < AT_R) {
        float a = p.bd[tid];
        for (int ci = 0; ci < AT_C; ++ci) a = fmaf(p.wd[tid * AT_C + ci], z[ci], a);
        g[tid] = a > 0.0f ? a : a * p.slope;
    }
    __syncthreads();
    if (tid == 0) {
        float u = p.bu[c];
        for (int j = 0; j < AT_R; ++j) u = fmaf(p.wu[c * AT_R + j], g[j], u);
        const float s = 1.0f / (1.0f + expf(-u));
        sgate = s;
        if (p.gate && k == 0) p.gate[n * AT_C + c] = s;
    }
    __syncthreads();
    const float s = sgate;
    const float* xp = p.x + (long long)n * p.xImage + (long long)c * p.xPlane;
    const float* tp = p.t + (long long)n * p.tImage + (long long)c * p.tPlane;
    float* yp = p.y + (long long)n * p.yImage + (long long)c * p.yPlane;
    const long long lo = (long long)k * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;
    unsigned mag = 0;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* x4 = reinterpret_cast<const float4*>(xp + lo);
        const float4* t4 = reinterpret_cast<const float4*>(tp + lo);
        float4* y4 = reinterpret_cast<float4*>(yp + lo);
        for (long long q = tid; q < quads; q += AT_THREADS) {
            const float4 a = x4[q], b = t4[q];
            float4 v;
            v.x = scale_add(a.x, b.x, s);
            v.y = scale_add(a.y, b.y, s);
            v.z = scale_add(a.z, b.z, s);
            v.w = scale_add(a.w, b.w, s);
            mag = isr_umax(isr_umax(mag, isr_umax(isr_mag(v.x), isr_mag(v.y))), isr_umax(isr_mag(v.z), isr_mag(v.w)));
            y4[q] = v;
        }
        const long long rest = lo + 4 * quads + tid;
        if (tid < 3 && rest < hi) {
            const float v = scale_add(xp[rest], tp[rest], s);
            mag = isr_umax(mag, isr_mag(v));
            yp[rest] = v;
        }
    } else {
        for (long long i = lo + tid; i < hi; i += AT_THREADS) {
            const float v = scale_add(xp[i], tp[i], s);
            mag = isr_umax(mag, isr_mag(v));
            yp[i] = v;
        }
    }
    isr_range_note(p.absmax, mag);
}

// ---- backward of the channel attention ----------------------------------------------------------------------------------------------

struct GradSumParams {
    const float* dy; long long dyPlane, dyImage;
    const float* t; long long tPlane, tImage;
    long long hw, chunk;
    int S, vec;
    double* ws;
};

// channel_pool_kernel over the products dy * t, each rounded to fp32 once
__global__ void __launch_bounds__(AT_THREADS) gate_grad_sum_kernel(const GradSumParams p)
{
    __shared__ double sh[AT_THREADS];
    const int s = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const float* gp = p.dy + (long long)n * p.dyImage + (long long)c * p.dyPlane;
    const float* tp = p.t + (long long)n * p.tImage + (long long)c * p.tPlane;
    const long long lo = (long long)s * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;
    double acc = 0.0;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* g4 = reinterpret_cast<const float4*>(gp + lo);
        const float4* t4 = reinterpret_cast<const float4*>(tp + lo);
        for (long long q = tid; q < quads; q += AT_THREADS) {
            const float4 a = g4[q], b = t4[q];
            const float mx = a.x * b.x, my = a.y * b.y, mz = a.z * b.z, mw = a.w * b.w;
            acc = acc + (double)mx;
            acc = acc + (double)my;
            acc = acc + (double)mz;
            acc = acc + (double)mw;
        }
        const long long rest = lo + 4 * quads + tid;
        if (tid < 3 && rest < hi) { const float m = gp[rest] * tp[rest]; acc = acc + (double)m; }
    } else {
        for (long long i = lo + tid; i < hi; i += AT_THREADS) { const float m = gp[i] * tp[i]; acc = acc + (double)m; }
    }
    tree_sum(sh, acc, tid);
    if (tid == 0) p.ws[((long long)n * AT_C + c) * p.S + s] = sh[0];
}

// what the perceptron's backward of one image leaves in LDS
struct PerceptronGrad {
    float z[AT_C];       // the saved mean
    float du[AT_C];      // ds * s * (1 - s)
    float a[AT_R], g[AT_R], da[AT_R];
};

struct PerceptronOperands {
    const double* ws; int S;                 // the slab sums of dy * t
    const float* mean; const float* gate;    // z and s [N][64] of the forward
    const float* wd; const float* bd; const float* wu;
    float slope;
};

// Every thread of the workgroup calls this; L is complete (and the workgroup synchronised) on return.
__device__ __forceinline__ void perceptron_backward(PerceptronGrad& L, const PerceptronOperands& o, int n, int tid)
{
    if (tid < AT_C) {
        const double* q = o.ws + ((long long)n * AT_C + tid) * o.S;
        double sum = 0.0;
        for (int s = 0; s < o.S; ++s) sum = sum + q[s];
        const float ds = (float)sum;
        const float s = o.gate[n * AT_C + tid];
        const float om = 1.0f - s;
        const float sp = s * om;
        L.z[tid] = o.mean[n * AT_C + tid];
        L.du[tid] = ds * sp;
    }
    __syncthreads();
    if (tid < AT_R) {
        float a = o.bd[tid];
        for (int ci = 0; ci < AT_C; ++ci) a = fmaf(o.wd[tid * AT_C + ci], L.z[ci], a);
        double sum = 0.0;                                  // (64 terms of either sign: summed in fp64, every product exact)
        for (int c = 0; c < AT_C; ++c) sum = fma((double)o.wu[c * AT_R + tid], (double)L.du[c], sum);
        const float dg = (float)sum;
        L.a[tid] = a;
        L.g[tid] = a > 0.0f ? a : a * o.slope;
        L.da[tid] = a > 0.0f ? dg : dg * o.slope;
    }
    __syncthreads();
}

struct GateBackParams {
    const float* dy; float* dt;
    long long dyPlane, dyImage, dtPlane, dtImage;
    long long hw, chunk;
    PerceptronOperands o;
    int vec;
};

__global__ void __launch_bounds__(AT_THREADS) gate_backward_kernel(const GateBackParams p)
{
    __shared__ PerceptronGrad L;
    __shared__ float sq;
    const int k = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    perceptron_backward(L, p.o, n, tid);
    if (tid == 0) {
        float dz = 0.0f;
        for (int j = 0; j < AT_R; ++j) dz = fmaf(p.o.wd[j * AT_C + c], L.da[j], dz);
        sq = (float)((double)dz / (double)p.hw);
    }
    __syncthreads();
    const float q = sq, s = p.o.gate[n * AT_C + c];
    const float* gp = p.dy + (long long)n * p.dyImage + (long long)c * p.dyPlane;
    float* dp = p.dt + (long long)n * p.dtImage + (long long)c * p.dtPlane;
    const long long lo = (long long)k * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* g4 = reinterpret_cast<const float4*>(gp + lo);
        float4* d4 = reinterpret_cast<float4*>(dp + lo);
        for (long long i = tid; i < quads; i += AT_THREADS) {
            const float4 a = g4[i];
            float4 v;
            v.x = scale_add(q, a.x, s);
            v.y = scale_add(q, a.y, s);
            v.z = scale_add(q, a.z, s);
            v.w = scale_add(q, a.w, s);
            d4[i] = v;
        }
        const long long rest = lo + 4 * quads + tid;
        if (tid < 3 && rest < hi) dp[rest] = scale_add(q, gp[rest], s);
    } else {
        for (long long i = lo + tid; i < hi; i += AT_THREADS) dp[i] = scale_add(q, gp[i], s);
    }
}

struct ParamGradParams {
    PerceptronOperands o;
    int N;
    float* dWd; float* dbd; float* dWu; float* dbu;
};

// ONE workgroup.  Thread tid owns dWu[tid / 4][tid % 4] and dWd[tid / 64][tid % 64]; threads 0 .. 63 also dbu, 64 .. 67 dbd.
__global__ void __launch_bounds__(AT_THREADS) gate_param_grad_kernel(const ParamGradParams p)
{
    __shared__ PerceptronGrad L;
    const int tid = threadIdx.x;
    double up = 0.0, down = 0.0, bias = 0.0;
    for (int n = 0; n < p.N; ++n) {
        perceptron_backward(L, p.o, n, tid);
        up = fma((double)L.du[tid >> 2], (double)L.g[tid & 3], up);
        down = fma((double)L.da[tid >> 6], (double)L.z[tid & 63], down);
        if (tid < AT_C) bias = bias + (double)L.du[tid];
        else if (tid < AT_C + AT_R) bias = bias + (double)L.da[tid - AT_C];
        __syncthreads();                                   // L is rewritten for the next image
    }
    p.dWu[tid] = (float)up;
    p.dWd[tid] = (float)down;
    if (tid < AT_C) p.dbu[tid] = (float)bias;
    else if (tid < AT_C + AT_R) p.dbd[tid - AT_C] = (float)bias;
}

struct TailParams {
    const float* f; long long fPlane, fImage;
    const float* w; const float* b;
    float* out; long long outPlane, outImage;
    int h, w_, Cout;
    int clamp, vecIn, vecOut;
};

// stage: channel ch = 16 ci + 4 i + j of low-resolution patch pixel (ly, lx) -> P[ci][4 ly + i][4 lx + j]; zero outside the image
__device__ __forceinline__ void stage_shuffled(float* P, const float* f, long long fPlane, int h, int w, int y0, int x0, int vecIn, int tid)
{
    if (vecIn) {
        // one wave per (ci, ly): its lanes are the 16 channels 16 ci + 4 i + j (j fastest) x the 4 quads of the row
        for (int e = tid; e < AT_C * TP_H * (TL_W / 4); e += AT_THREADS) {
            const int j = e & 3, q = (e >> 2) & 3, i = (e >> 4) & 3, ly = (e >> 6) % TP_H, ci = (e >> 6) / TP_H;
            const int ch = 16 * ci + 4 * i + j;
            const int gy = y0 - 1 + ly, gx = x0 + 4 * q;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (gy >= 0 && gy < h && gx < w) v = *reinterpret_cast<const float4*>(f + (long long)ch * fPlane + (long long)gy * w + gx);
            float* d = P + ((ch >> 4) * TS_H + 4 * ly + ((ch >> 2) & 3)) * TS_STRIDE + 4 * (1 + 4 * q) + (ch & 3);
            d[0] = v.x; d[4] = v.y; d[8] = v.z; d[12] = v.w;
        }
        for (int e = tid; e < AT_C * TP_H * 2; e += AT_THREADS) {
            const int side = e & 1, ly = (e >> 1) % TP_H, ch = (e >> 1) / TP_H;
            const int lx = side ? TP_W - 1 : 0;
            const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
            float v = 0.0f;
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = f[(long long)ch * fPlane + (long long)gy * w + gx];
            P[((ch >> 4) * TS_H + 4 * ly + ((ch >> 2) & 3)) * TS_STRIDE + 4 * lx + (ch & 3)] = v;
        }
    } else {
        for (int e = tid; e < AT_C * TP_H * TP_W; e += AT_THREADS) {
            const int lx = e % TP_W, ly = (e / TP_W) % TP_H, ch = e / (TP_W * TP_H);
            const int gy = y0 - 1 + ly, gx = x0 - 1 + lx;
            float v = 0.0f;
            if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = f[(long long)ch * fPlane + (long long)gy * w + gx];
            P[((ch >> 4) * TS_H + 4 * ly + ((ch >> 2) & 3)) * TS_STRIDE + 4 * lx + (ch & 3)] = v;
        }
    }
}

// COUT: the accumulators a thread carries (3: the colour networks; 8: anything up to eight channels, stores masked by p.Cout)
template <int COUT>
__global__ void __launch_bounds__(AT_THREADS) shuffle_tail_kernel(const TailParams p)
{
    __shared__ __attribute__((aligned(16))) float P[4 * TS_H * TS_STRIDE];      // [ci][4 ly + i][4 lx + j]: 48 640 bytes
    __shared__ float sw[TAIL_MAX_COUT * 36 + TAIL_MAX_COUT];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * TL_H, x0 = blockIdx.x * TL_W;
    const int h = p.h, w = p.w_;
    const float* f = p.f + (long long)n * p.fImage;
    for (int e = tid; e < TAIL_MAX_COUT * 36 + TAIL_MAX_COUT; e += AT_THREADS) {
        float v = 0.0f;
        if (e < TAIL_MAX_COUT * 36) { if (e < p.Cout * 36) v = p.w[e]; }
        else if (e - TAIL_MAX_COUT * 36 < p.Cout && p.b) v = p.b[e - TAIL_MAX_COUT * 36];
        sw[e] = v;
    }
    stage_shuffled(P, f, p.fPlane, h, w, y0, x0, p.vecIn, tid);
    __syncthreads();
    const int qx = tid & 15, ry = tid >> 4;
    const int H4 = 4 * h, W4 = 4 * w;
    const int GX = 4 * x0 + 4 * qx;
    float* out = p.out + (long long)n * p.outImage;
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int Y = ry + 16 * half;                      // row of the 32 x 64 high-resolution tile
        const int GY = 4 * y0 + Y;
        if (GY >= H4 || GX >= W4) continue;                // (W4 is a multiple of four: a quad is inside or outside as a whole)
        float acc[COUT][4];
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            const float b = sw[TAIL_MAX_COUT * 36 + co];
            acc[co][0] = b; acc[co][1] = b; acc[co][2] = b; acc[co][3] = b;
        }
        // (one input channel at a time: fully unrolled, the compiler keeps all 36 Cout weights in registers -- 406 VGPRs for Cout = 3,
        //  one wave per SIMD, and scratch for Cout = 8)
#pragma unroll 1
        for (int ci = 0; ci < 4; ++ci) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                // patch row Y + 4 + ky - 1, patch columns 4 qx + 4 - 1 .. + 4
                const float* row = P + (ci * TS_H + Y + 3 + ky) * TS_STRIDE + 4 * qx + 3;
                float v[6];
                v[0] = row[0];
                const float4 m = *reinterpret_cast<const float4*>(row + 1);
                v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w;
                v[5] = row[5];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
                    for (int co = 0; co < COUT; ++co) {
                        const float wt = sw[co * 36 + ci * 9 + ky * 3 + kx];
#pragma unroll
                        for (int px = 0; px < 4; ++px) acc[co][px] = fmaf(wt, v[px + kx], acc[co][px]);
                    }
                }
            }
        }
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            if (co >= p.Cout) break;
            if (p.clamp) {
#pragma unroll
                for (int px = 0; px < 4; ++px) { const float v = acc[co][px]; acc[co][px] = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v); }
            }
            float* o = out + (long long)co * p.outPlane + (long long)GY * W4 + GX;
            if (p.vecOut) *reinterpret_cast<float4*>(o) = make_float4(acc[co][0], acc[co][1], acc[co][2], acc[co][3]);
            else { o[0] = acc[co][0]; o[1] = acc[co][1]; o[2] = acc[co][2]; o[3] = acc[co][3]; }
        }
    }
}

// ---- backward of the tail -----------------------------------------------------------------------------------------------------------

struct TailDgradParams {
    const float* dout; long long doutPlane, doutImage;
    const float* w;
    float* df; long long dfPlane, dfImage;
    int h, w_, Cout, vecIn;
};

// Thread (ly, lx, half) = (tid / 16 % 8, tid % 16, tid / 128): the 4 x 4 high-resolution pixels of low-resolution pixel (ly, lx) of the tile,
// channels ci = 2 half and 2 half + 1 of P.  Stores are per element (the 16 lanes of a row write 64 contiguous bytes of one plane of df).
__global__ void __launch_bounds__(AT_THREADS) shuffle_tail_dgrad_kernel(const TailDgradParams p)
{
    __shared__ __attribute__((aligned(16))) float D[TD_CO * TD_H * TD_STRIDE];      // [co % 4][1 + Y][1 + X]: 36 992 bytes
    __shared__ float sw[TAIL_MAX_COUT * 36];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * TL_H, x0 = blockIdx.x * TL_W;
    const int h = p.h, w = p.w_, H4 = 4 * h, W4 = 4 * w;
    const float* dout = p.dout + (long long)n * p.doutImage;
    for (int e = tid; e < TAIL_MAX_COUT * 36; e += AT_THREADS) sw[e] = e < p.Cout * 36 ? p.w[e] : 0.0f;
    const int lx = tid & 15, ly = (tid >> 4) & 7, half = tid >> 7;
    float acc[2][4][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[a][i][j] = 0.0f;
#pragma unroll 1
    for (int co0 = 0; co0 < p.Cout; co0 += TD_CO) {
        __syncthreads();                                   // (the chunk before has been read; sw is written)
        // stage: dout[co0 + c][4 y0 - 1 + r][4 x0 - 1 + cc] -> D[c][r][cc]; zero outside the image and behind the last channel
        if (p.vecIn) {
            for (int e = tid; e < TD_CO * TD_H * TL_W; e += AT_THREADS) {      // (TL_W quads of four high-resolution pixels per row)
                const int q = e & 15, r = (e >> 4) % TD_H, c = (e >> 4) / TD_H;
                const int gy = 4 * y0 - 1 + r, gx = 4 * x0 + 4 * q;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (co0 + c < p.Cout && gy >= 0 && gy < H4 && gx < W4)
                    v = *reinterpret_cast<const float4*>(dout + (long long)(co0 + c) * p.doutPlane + (long long)gy * W4 + gx);
                float* d = D + (c * TD_H + r) * TD_STRIDE + 1 + 4 * q;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
            for (int e = tid; e < TD_CO * TD_H * 2; e += AT_THREADS) {
                const int side = e & 1, r = (e >> 1) % TD_H, c = (e >> 1) / TD_H;
                const int cc = side ? TD_W - 1 : 0;
                const int gy = 4 * y0 - 1 + r, gx = 4 * x0 - 1 + cc;
                float v = 0.0f;
                if (co0 + c < p.Cout && gy >= 0 && gy < H4 && gx >= 0 && gx < W4) v = dout[(long long)(co0 + c) * p.doutPlane + (long long)gy * W4 + gx];
                D[(c * TD_H + r) * TD_STRIDE + cc] = v;
            }
        } else {
            for (int e = tid; e < TD_CO * TD_H * TD_W; e += AT_THREADS) {
                const int cc = e % TD_W, r = (e / TD_W) % TD_H, c = e / (TD_W * TD_H);
                const int gy = 4 * y0 - 1 + r, gx = 4 * x0 - 1 + cc;
                float v = 0.0f;
                if (co0 + c < p.Cout && gy >= 0 && gy < H4 && gx >= 0 && gx < W4) v = dout[(long long)(co0 + c) * p.doutPlane + (long long)gy * W4 + gx];
                D[(c * TD_H + r) * TD_STRIDE + cc] = v;
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int c = 0; c < TD_CO; ++c) {
            const int co = co0 + c;
            if (co >= p.Cout) break;
            // pixels 4 ly - 1 .. 4 ly + 4 of the tile in both directions: rows 4 ly .. 4 ly + 5, columns 4 lx .. 4 lx + 5 of D
            float v[6][6];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const float* row = D + (c * TD_H + 4 * ly + r) * TD_STRIDE + 4 * lx;
                const float4 m = *reinterpret_cast<const float4*>(row);
                const float2 t = *reinterpret_cast<const float2*>(row + 4);
                v[r][0] = m.x; v[r][1] = m.y; v[r][2] = m.z; v[r][3] = m.w; v[r][4] = t.x; v[r][5] = t.y;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
#pragma unroll
                    for (int a = 0; a < 2; ++a) {
                        const float wt = sw[co * 36 + (2 * half + a) * 9 + (2 - ky) * 3 + (2 - kx)];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[a][i][j] = fmaf(wt, v[i + ky][j + kx], acc[a][i][j]);
                    }
                }
            }
        }
    }
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= h || gx >= w) return;
    float* df = p.df + (long long)n * p.dfImage + (long long)gy * w + gx;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) df[(long long)(16 * (2 * half + a) + 4 * i + j) * p.dfPlane] = acc[a][i][j];
}

struct TailWgradParams {
    const float* dout; long long doutPlane, doutImage;
    const float* f; long long fPlane, fImage;
    int h, w_, Cout, vecIn, vecOut;
    double* ws;                  // [tiles][Cout][TW_TERMS]
};

// The forward's tile and thread layout: thread (ry, qx) = (tid / 16, tid % 16) owns pixels (ry + 16 half, 4 qx .. 4 qx + 3) of the 32 x 64 tile.
__global__ void __launch_bounds__(AT_THREADS) shuffle_tail_wgrad_kernel(const TailWgradParams p)
{
    __shared__ __attribute__((aligned(16))) float P[4 * TS_H * TS_STRIDE];
    __shared__ double red[AT_THREADS / 64][TW_TERMS];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int y0 = blockIdx.y * TL_H, x0 = blockIdx.x * TL_W;
    const int h = p.h, w = p.w_, H4 = 4 * h, W4 = 4 * w;
    const long long tile = ((long long)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    stage_shuffled(P, p.f + (long long)n * p.fImage, p.fPlane, h, w, y0, x0, p.vecIn, tid);
    __syncthreads();
    const int qx = tid & 15, ry = tid >> 4;
    const int GX = 4 * x0 + 4 * qx;
    const float* dout = p.dout + (long long)n * p.doutImage;
#pragma unroll 1
    for (int co = 0; co < p.Cout; ++co) {
        double acc[TW_TERMS];
#pragma unroll
        for (int t = 0; t < TW_TERMS; ++t) acc[t] = 0.0;
#pragma unroll 1
        for (int half = 0; half < 2; ++half) {
            const int Y = ry + 16 * half;
            const int GY = 4 * y0 + Y;
            if (GY >= H4 || GX >= W4) continue;            // (W4 is a multiple of four: a quad is inside or outside as a whole)
            const float* g = dout + (long long)co * p.doutPlane + (long long)GY * W4 + GX;
            float d[4];
            if (p.vecOut) { const float4 m = *reinterpret_cast<const float4*>(g); d[0] = m.x; d[1] = m.y; d[2] = m.z; d[3] = m.w; }
            else { d[0] = g[0]; d[1] = g[1]; d[2] = g[2]; d[3] = g[3]; }
#pragma unroll
            for (int px = 0; px < 4; ++px) acc[36] = acc[36] + (double)d[px];
#pragma unroll
            for (int ci = 0; ci < 4; ++ci) {
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const float* row = P + (ci * TS_H + Y + 3 + ky) * TS_STRIDE + 4 * qx + 3;
                    float v[6];
                    v[0] = row[0];
                    const float4 m = *reinterpret_cast<const float4*>(row + 1);
                    v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w;
                    v[5] = row[5];
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int px = 0; px < 4; ++px)
                            acc[ci * 9 + ky * 3 + kx] = fma((double)d[px], (double)v[px + kx], acc[ci * 9 + ky * 3 + kx]);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < TW_TERMS; ++t) {
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) acc[t] = acc[t] + __shfl_xor(acc[t], off, 64);
            if ((tid & 63) == 0) red[tid >> 6][t] = acc[t];
        }
        __syncthreads();
        if (tid < TW_TERMS) p.ws[(tile * p.Cout + co) * TW_TERMS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        __syncthreads();                                   // red is rewritten for the next channel
    }
}

// thread e = co * 37 + term: the tiles' partials in index order, one rounding
__global__ void shuffle_tail_wgrad_sum_kernel(const double* ws, int tiles, int Cout, float* dw, float* db)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Cout * TW_TERMS) return;
    const int co = e / TW_TERMS, t = e % TW_TERMS;
    double sum = 0.0;
    for (int k = 0; k < tiles; ++k) sum = sum + ws[(long long)k * Cout * TW_TERMS + e];
    if (t < 36) dw[co * 36 + t] = (float)sum;
    else if (db) db[co] = (float)sum;
}

bool tail_supported(int N, int C, int Cout, int h, int w, long long fPlane, long long fImage, long long outPlane, long long outImage)
{
    if (N <= 0 || N > 65535 || C != AT_C || Cout <= 0 || Cout > TAIL_MAX_COUT || h <= 0 || w <= 0) return false;
    const long long hw = (long long)h * w;
    if (fPlane < hw || fImage < (long long)AT_C * fPlane || outPlane < 16 * hw || outImage < (long long)Cout * outPlane) return false;
    if ((h + TL_H - 1) / TL_H > 65535) return false;
    return fImage * 4 < (1ll << 31) && outImage * 4 < (1ll << 31);
}

long long tail_tiles(int N, int h, int w) { return (long long)N * ((h + TL_H - 1) / TL_H) * ((w + TL_W - 1) / TL_W); }

}  // namespace

extern "C" {

int isrChannelPoolSlabs(int N, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0) return -1;
    return pool_slabs(N, H, W);
}

int isrChannelPoolSupported(int N, int C, int H, int W, long long plane, long long image)
{
    return attention_supported(N, C, AT_R, H, W, plane, image) ? 1 : 0;
}

int isrChannelGateScaleAddSupported(int N, int C, int R, int H, int W, long long plane, long long image)
{
    return attention_supported(N, C, R, H, W, plane, image) ? 1 : 0;
}

int isrChannelPool(const float* t, long long tPlane, long long tImage, int N, int C, int H, int W, int S, double* workspace, void* stream)
{
    if (!t || !workspace || N <= 0 || H <= 0 || W <= 0) return -1;
    if (!attention_supported(N, C, AT_R, H, W, tPlane, tImage)) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    PoolParams p;
    p.t = t; p.tPlane = tPlane; p.tImage = tImage;
    p.hw = (long long)H * W; p.chunk = pool_chunk(p.hw, S); p.S = S;
    p.vec = (aligned16(t) && (tPlane & 3) == 0 && (tImage & 3) == 0) ? 1 : 0;
    p.ws = workspace;
    return isr_launch(ISR_VARIANT_CHANNEL_POOL, 0.0, channel_pool_kernel, dim3((unsigned)S, AT_C, (unsigned)N), dim3(AT_THREADS), 0, (hipStream_t)stream, p);
}

int isrChannelPoolMean(const double* workspace, int N, int C, int H, int W, int S, float* mean, void* stream)
{
    if (!workspace || !mean || N <= 0 || H <= 0 || W <= 0) return -1;
    if (C != AT_C || N > 65535) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    const int planes = N * AT_C;
    hipLaunchKernelGGL(channel_mean_kernel, dim3((planes + AT_THREADS - 1) / AT_THREADS), dim3(AT_THREADS), 0, (hipStream_t)stream,
                       workspace, S, (long long)H * W, planes, mean);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int isrChannelGateScaleAdd(const float* x, const float* t, float* y, long long xPlane, long long xImage, long long tPlane, long long tImage,
                           long long yPlane, long long yImage, const double* workspace, int S, const float* wDown, const float* bDown,
                           const float* wUp, const float* bUp, float slope, float* gate, int N, int C, int R, int H, int W, void* stream)
{
    unsigned* const rangeFlag = isr_take_range_flag();       // taken first: an error return must not leave it armed
    if (!x || !t || !y || !workspace || !wDown || !bDown || !wUp || !bUp || N <= 0 || H <= 0 || W <= 0) return -1;
    if (!attention_supported(N, C, R, H, W, xPlane, xImage) || !attention_supported(N, C, R, H, W, tPlane, tImage)
        || !attention_supported(N, C, R, H, W, yPlane, yImage)) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    GateParams p;
    p.x = x; p.t = t; p.y = y;
    p.xPlane = xPlane; p.xImage = xImage; p.tPlane = tPlane; p.tImage = tImage; p.yPlane = yPlane; p.yImage = yImage;
    p.hw = (long long)H * W; p.chunk = AT_CHUNK;
    p.ws = workspace; p.S = S;
    p.wd = wDown; p.bd = bDown; p.wu = wUp; p.bu = bUp; p.slope = slope; p.gate = gate;
    p.vec = (aligned16(x) && aligned16(t) && aligned16(y) && ((xPlane | xImage | tPlane | tImage | yPlane | yImage) & 3) == 0) ? 1 : 0;
    p.absmax = rangeFlag;
    const long long chunks = (p.hw + AT_CHUNK - 1) / AT_CHUNK;
    return isr_launch(ISR_VARIANT_GATE_SCALE_ADD, 0.0, gate_scale_add_kernel, dim3((unsigned)chunks, AT_C, (unsigned)N), dim3(AT_THREADS), 0,
                      (hipStream_t)stream, p);
}

int isrChannelAttentionBackwardSupported(int N, int C, int R, int H, int W, long long plane, long long image)
{
    return attention_supported(N, C, R, H, W, plane, image) ? 1 : 0;
}

int isrChannelGateGradSums(const float* dy, long long dyPlane, long long dyImage, const float* t, long long tPlane, long long tImage,
                           int N, int C, int H, int W, int S, double* workspace, void* stream)
{
    if (!dy || !t || !workspace || N <= 0 || H <= 0 || W <= 0) return -1;
    if (!attention_supported(N, C, AT_R, H, W, dyPlane, dyImage) || !attention_supported(N, C, AT_R, H, W, tPlane, tImage)) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    GradSumParams p;
    p.dy = dy; p.dyPlane = dyPlane; p.dyImage = dyImage; p.t = t; p.tPlane = tPlane; p.tImage = tImage;
    p.hw = (long long)H * W; p.chunk = pool_chunk(p.hw, S); p.S = S;
    p.vec = (aligned16(dy) && aligned16(t) && ((dyPlane | dyImage | tPlane | tImage) & 3) == 0) ? 1 : 0;
    p.ws = workspace;
    return isr_launch(ISR_VARIANT_GATE_GRAD_SUM, 0.0, gate_grad_sum_kernel, dim3((unsigned)S, AT_C, (unsigned)N), dim3(AT_THREADS), 0,
                      (hipStream_t)stream, p);
}

int isrChannelGateScaleBackward(const float* dy, long long dyPlane, long long dyImage, float* dt, long long dtPlane, long long dtImage,
                                const double* workspace, int S, const float* mean, const float* gate, const float* wDown, const float* bDown,
                                const float* wUp, float slope, int N, int C, int R, int H, int W, void* stream)
{
    if (!dy || !dt || !workspace || !mean || !gate || !wDown || !bDown || !wUp || N <= 0 || H <= 0 || W <= 0) return -1;
    if (!attention_supported(N, C, R, H, W, dyPlane, dyImage) || !attention_supported(N, C, R, H, W, dtPlane, dtImage)) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    GateBackParams p;
    p.dy = dy; p.dt = dt; p.dyPlane = dyPlane; p.dyImage = dyImage; p.dtPlane = dtPlane; p.dtImage = dtImage;
    p.hw = (long long)H * W; p.chunk = AT_CHUNK;
    p.o.ws = workspace; p.o.S = S; p.o.mean = mean; p.o.gate = gate; p.o.wd = wDown; p.o.bd = bDown; p.o.wu = wUp; p.o.slope = slope;
    p.vec = (aligned16(dy) && aligned16(dt) && ((dyPlane | dyImage | dtPlane | dtImage) & 3) == 0) ? 1 : 0;
    const long long chunks = (p.hw + AT_CHUNK - 1) / AT_CHUNK;
    return isr_launch(ISR_VARIANT_GATE_BACKWARD, 0.0, gate_backward_kernel, dim3((unsigned)chunks, AT_C, (unsigned)N), dim3(AT_THREADS), 0,
                      (hipStream_t)stream, p);
}

int isrChannelGateParamGrad(const double* workspace, int S, const float* mean, const float* gate, const float* wDown, const float* bDown,
                            const float* wUp, float slope, float* dWDown, float* dBDown, float* dWUp, float* dBUp, int N, int C, int R,
                            int H, int W, void* stream)
{
    if (!workspace || !mean || !gate || !wDown || !bDown || !wUp || !dWDown || !dBDown || !dWUp || !dBUp || N <= 0 || H <= 0 || W <= 0) return -1;
    if (C != AT_C || R != AT_R || N > 65535) return -3;
    if (S != pool_slabs(N, H, W)) return -1;
    ParamGradParams p;
    p.o.ws = workspace; p.o.S = S; p.o.mean = mean; p.o.gate = gate; p.o.wd = wDown; p.o.bd = bDown; p.o.wu = wUp; p.o.slope = slope;
    p.N = N; p.dWd = dWDown; p.dbd = dBDown; p.dWu = dWUp; p.dbu = dBUp;
    return isr_launch(ISR_VARIANT_GATE_PARAM_GRAD, 0.0, gate_param_grad_kernel, dim3(1), dim3(AT_THREADS), 0, (hipStream_t)stream, p);
}

int isrShuffleTailBackwardSupported(int N, int C, int Cout, int h, int w, long long fPlane, long long fImage, long long outPlane, long long outImage)
{
    return tail_supported(N, C, Cout, h, w, fPlane, fImage, outPlane, outImage) && tail_tiles(N, h, w) <= TW_MAX_TILES ? 1 : 0;
}

int isrShuffleTailGradTiles(int N, int h, int w)
{
    if (N <= 0 || h <= 0 || w <= 0) return -1;
    const long long tiles = tail_tiles(N, h, w);
    return tiles <= TW_MAX_TILES ? (int)tiles : -3;
}

int isrShuffleTailDataGrad(const float* dout, long long doutPlane, long long doutImage, const float* weight, float* df, long long dfPlane,
                           long long dfImage, int N, int C, int Cout, int h, int w, void* stream)
{
    if (!dout || !weight || !df || N <= 0 || h <= 0 || w <= 0) return -1;
    if (!tail_supported(N, C, Cout, h, w, dfPlane, dfImage, doutPlane, doutImage)) return -3;
    TailDgradParams p;
    p.dout = dout; p.doutPlane = doutPlane; p.doutImage = doutImage; p.w = weight;
    p.df = df; p.dfPlane = dfPlane; p.dfImage = dfImage;
    p.h = h; p.w_ = w; p.Cout = Cout;
    p.vecIn = (aligned16(dout) && (doutPlane & 3) == 0 && (doutImage & 3) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((w + TL_W - 1) / TL_W), (unsigned)((h + TL_H - 1) / TL_H), (unsigned)N);
    const double flops = 2.0 * 36 * Cout * 16.0 * (double)N * h * w;
    return isr_launch(ISR_VARIANT_SHUFFLE_TAIL_DGRAD, flops, shuffle_tail_dgrad_kernel, grid, dim3(AT_THREADS), 0, (hipStream_t)stream, p);
}

int isrShuffleTailWeightGrad(const float* dout, long long doutPlane, long long doutImage, const float* f, long long fPlane, long long fImage,
                             int N, int C, int Cout, int h, int w, int tiles, double* workspace, float* dWeight, float* dBias, void* stream)
{
    if (!dout || !f || !workspace || !dWeight || N <= 0 || h <= 0 || w <= 0) return -1;
    if (!tail_supported(N, C, Cout, h, w, fPlane, fImage, doutPlane, doutImage) || tail_tiles(N, h, w) > TW_MAX_TILES) return -3;
    if (tiles != (int)tail_tiles(N, h, w)) return -1;
    TailWgradParams p;
    p.dout = dout; p.doutPlane = doutPlane; p.doutImage = doutImage; p.f = f; p.fPlane = fPlane; p.fImage = fImage;
    p.h = h; p.w_ = w; p.Cout = Cout;
    p.vecIn = (aligned16(f) && (w & 3) == 0 && (fPlane & 3) == 0 && (fImage & 3) == 0) ? 1 : 0;
    p.vecOut = (aligned16(dout) && (doutPlane & 3) == 0 && (doutImage & 3) == 0) ? 1 : 0;
    p.ws = workspace;
    const dim3 grid((unsigned)((w + TL_W - 1) / TL_W), (unsigned)((h + TL_H - 1) / TL_H), (unsigned)N);
    const double flops = 2.0 * 36 * Cout * 16.0 * (double)N * h * w;
    const int rc = isr_launch(ISR_VARIANT_SHUFFLE_TAIL_WGRAD, flops, shuffle_tail_wgrad_kernel, grid, dim3(AT_THREADS), 0, (hipStream_t)stream, p);
    if (rc != 0) return rc;
    const int terms = Cout * TW_TERMS;
    return isr_launch(ISR_VARIANT_SHUFFLE_TAIL_WGRAD_SUM, 0.0, shuffle_tail_wgrad_sum_kernel, dim3((unsigned)((terms + 63) / 64)), dim3(64), 0,
                      (hipStream_t)stream, (const double*)workspace, tiles, Cout, dWeight, dBias);
}

int isrShuffleTailColourSupported(int N, int C, int Cout, int h, int w, long long fPlane, long long fImage, long long outPlane, long long outImage)
{
    return tail_supported(N, C, Cout, h, w, fPlane, fImage, outPlane, outImage) ? 1 : 0;
}

int isrShuffleTailColour(const float* f, long long fPlane, long long fImage, const float* weight, const float* bias, float* out,
                         long long outPlane, long long outImage, int N, int C, int Cout, int h, int w, int clamp, void* stream)
{
    if (!f || !weight || !out || N <= 0 || h <= 0 || w <= 0) return -1;
    if (!tail_supported(N, C, Cout, h, w, fPlane, fImage, outPlane, outImage)) return -3;
    TailParams p;
    p.f = f; p.fPlane = fPlane; p.fImage = fImage; p.w = weight; p.b = bias;
    p.out = out; p.outPlane = outPlane; p.outImage = outImage;
    p.h = h; p.w_ = w; p.Cout = Cout; p.clamp = clamp ? 1 : 0;
    p.vecIn = (aligned16(f) && (w & 3) == 0 && (fPlane & 3) == 0 && (fImage & 3) == 0) ? 1 : 0;
    p.vecOut = (aligned16(out) && (outPlane & 3) == 0 && (outImage & 3) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((w + TL_W - 1) / TL_W), (unsigned)((h + TL_H - 1) / TL_H), (unsigned)N);
    const double flops = 2.0 * 36 * Cout * 16.0 * (double)N * h * w;
    if (Cout == 3) return isr_launch(ISR_VARIANT_SHUFFLE_TAIL, flops, shuffle_tail_kernel<3>, grid, dim3(AT_THREADS), 0, (hipStream_t)stream, p);
    return isr_launch(ISR_VARIANT_SHUFFLE_TAIL, flops, shuffle_tail_kernel<8>, grid, dim3(AT_THREADS), 0, (hipStream_t)stream, p);
}

}  // extern "C"
