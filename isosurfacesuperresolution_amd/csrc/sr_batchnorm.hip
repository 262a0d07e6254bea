// Training-mode batch normalisation of the EnhanceNet residual blocks (models/enhancenet.py with use_bn; include/isr_sr_kernels.h:
// isrBatchNormStats, isrBatchNormApply, isrBatchNormGradSums, isrBatchNormBackward).  x, y, dy, dx and the residual are fp32
// [N][C][H][W], packed; M = N H W values per channel.  All six kernels are memory bound: 16-byte accesses where every base address is a
// multiple of 16 bytes and H W a multiple of four, a per-element path otherwise; no floating-point atomics; plain pointer stores.
// (In eval mode a batch-norm layer is folded into its convolution by ops.fold_batch_norm and none of this runs.)
//
//   forward of one layer, THREE launches:
//     batch_norm_stat_kernel         slab sums of x - k and (x - k)^2 in fp64 -> workspace double [C][N S][2]; a slab is a run of one
//                                    plane, k = k[c] the channel's first value x[0][c][0][0]
//     batch_norm_finish_kernel       the once-only work, its own tiny launch (one thread per channel): the N S partials in index order,
//                                    mean, invstd, and the in-place update of the running statistics
//     batch_norm_apply_kernel        y = (x - mean) invstd gamma + beta, then ReLU or + residual
//   backward, THREE launches (the skip's gradient IS dy: no launch):
//     batch_norm_grad_sum_kernel     slab sums of g and g xhat in fp64 -> workspace (the forward's slabs), g = dy (y > 0) for the ReLU form
//     batch_norm_grad_finish_kernel  one thread per channel: dgamma, dbeta and the two fp32 coefficients of the streaming pass
//     batch_norm_backward_kernel     dx = gamma invstd (g - sum g / M - xhat sum(g xhat) / M)
//
// ORDER OF THE ARITHMETIC (what the tests' bounds are derived from; nothing below is contracted or reassociated by the compiler:
// file-scope pragma, explicit fma):
//   sums   : d = (double)x - (double)k; a thread adds d and fma(d, d, .) over its elements in
//            index order in fp64, the workgroup's 256 pairs go through an LDS tree of fixed shape: a partial depends on the shape of the
//            tensor and its alignment class only -- two runs give the same bits.  The shift k keeps the one-pass variance below free of
//            cancellation for channels whose mean is large against their spread.
//   stats  : a = ((p[0] + p[1]) + ...) + p[N S - 1] for both sums, in fp64; u = a1 / M; mean = k + u; var = max(a2 / M - u u, 0) (biased);
//            invstd = 1 / sqrt(var + eps); mean and invstd are rounded to fp32 once and stored.
//   running: running_mean = (float)((1 - m) (double)running_mean + m mean), running_var likewise with var M / (M - 1), from the fp64
//            values: one rounding each.
//   xhat   : d = x - mean, xhat = d * invstd in fp32 (two roundings), the same in the forward and in both backward kernels.
//   y      : t = xhat * gamma, v = t + beta as two separately rounded operations; ReLU: v < 0 ? 0 : v; residual: v + r.
//   g sums : g xhat is fma((double)g, (double)xhat, .): the product is exact; threads, tree and partials as in `sums`.
//   params : b1 = sum g, b2 = sum g xhat from the partials in index order; dbeta = (float)b1, dgamma = (float)b2,
//            c1 = (float)(b1 / M), c2 = (float)(b2 / M).
//   dx     : a = g - c1, b = xhat * c2, e = a - b, dx = e * (gamma * invstd): four roundings and the one of gamma * invstd.
#include "sr_split_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_SLABS = 64;
constexpr int BN_SLAB_PIXELS = 4096;   // a slab is at least this long (except the only one of a plane)
constexpr int BN_STAT_GROUPS = 1024;   // N * C * S aims at this many workgroups (four per CU)
constexpr int BN_CHUNK = 8192;         // elements of one plane a streaming workgroup handles
constexpr int ISR_VARIANT_BN_STAT = 54;          // ops.VARIANT_NAMES
constexpr int ISR_VARIANT_BN_FINISH = 55;
constexpr int ISR_VARIANT_BN_APPLY = 56;
constexpr int ISR_VARIANT_BN_GRAD_SUM = 57;
constexpr int ISR_VARIANT_BN_GRAD_FINISH = 58;
constexpr int ISR_VARIANT_BN_BACKWARD = 59;

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool bn_supported(int N, int C, int H, int W)
{
    if (N <= 0 || N > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0) return false;
    const long long hw = (long long)H * W;
    if (hw > (1ll << 31) || (long long)N * hw < 2) return false;
    return (long long)N * C * hw < (1ll << 40);
}

long long bn_chunk(long long hw, int S) { return (((hw + S - 1) / S) + 3) / 4 * 4; }

int bn_slabs(int N, int C, int H, int W)
{
    const long long hw = (long long)H * W;
    long long s = (hw + BN_SLAB_PIXELS - 1) / BN_SLAB_PIXELS;
    const long long planes = (long long)N * C;
    const long long most = BN_STAT_GROUPS / planes > 1 ? BN_STAT_GROUPS / planes : 1;
    if (s > most) s = most;
    if (s > BN_MAX_SLABS) s = BN_MAX_SLABS;
    if (s < 1) s = 1;
    // slabs are whole 16-byte quads; the count that leaves none of them empty
    const long long chunk = bn_chunk(hw, (int)s);
    return (int)((hw + chunk - 1) / chunk);
}

// the workgroup's 256 pairs of fp64 sums through an LDS tree of fixed shape; the totals are in sh[0] and sh[BN_THREADS] afterwards
__device__ __forceinline__ void tree_sum2(double* sh, double a, double b, int tid)
{
    sh[tid] = a;
    sh[BN_THREADS + tid] = b;
    __syncthreads();
    for (int k = BN_THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) {
            sh[tid] = sh[tid] + sh[tid + k];
            sh[BN_THREADS + tid] = sh[BN_THREADS + tid] + sh[BN_THREADS + tid + k];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ float bn_xhat(float x, float mean, float invstd)
{
    const float d = x - mean;
    return d * invstd;
}

// act: 0 none, 1 ReLU; r is added afterwards where there is a residual
__device__ __forceinline__ float bn_value(float x, float mean, float invstd, float gamma, float beta, int relu)
{
    const float t = bn_xhat(x, mean, invstd) * gamma;
    const float v = t + beta;
    return relu ? (v < 0.0f ? 0.0f : v) : v;
}

struct StatParams {
    const float* x;
    long long hw, chunk;
    int C, S, vec;
    double* ws;                  // [C][N S][2]
};

// grid (S, C, N): slab s of plane (n, c)
__global__ void __launch_bounds__(BN_THREADS) batch_norm_stat_kernel(const StatParams p)
{
    __shared__ double sh[2 * BN_THREADS];
    const int s = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const double k = (double)p.x[(long long)c * p.hw];
    const float* plane = p.x + ((long long)n * p.C + c) * p.hw;
    const long long lo = (long long)s * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;
    double a1 = 0.0, a2 = 0.0;
    if (p.vec) {                                                     // (H W is a multiple of four: so is hi - lo)
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* q4 = reinterpret_cast<const float4*>(plane + lo);
        for (long long q = tid; q < quads; q += BN_THREADS) {
            const float4 v = q4[q];
            const double dx = (double)v.x - k, dy = (double)v.y - k, dz = (double)v.z - k, dw = (double)v.w - k;
            a1 = a1 + dx; a2 = fma(dx, dx, a2);
            a1 = a1 + dy; a2 = fma(dy, dy, a2);
            a1 = a1 + dz; a2 = fma(dz, dz, a2);
            a1 = a1 + dw; a2 = fma(dw, dw, a2);
        }
    } else {
        for (long long i = lo + tid; i < hi; i += BN_THREADS) {
            const double d = (double)plane[i] - k;
            a1 = a1 + d; a2 = fma(d, d, a2);
        }
    }
    tree_sum2(sh, a1, a2, tid);
    if (tid == 0) {
        double* o = p.ws + (((long long)c * gridDim.z + n) * p.S + s) * 2;
        o[0] = sh[0];
        o[1] = sh[BN_THREADS];
    }
}

struct StatFinishParams {
    const float* x;
    const double* ws;
    long long hw;
    int C, parts;                // parts = N S
    double count, eps, momentum; // count = M
    float* mean; float* invstd;
    float* runningMean; float* runningVar;       // NULL: not tracked
};

__global__ void __launch_bounds__(BN_THREADS) batch_norm_finish_kernel(const StatFinishParams p)
{
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c >= p.C) return;
    const double* q = p.ws + (long long)c * p.parts * 2;
    double a1 = 0.0, a2 = 0.0;
    for (int i = 0; i < p.parts; ++i) { a1 = a1 + q[2 * i]; a2 = a2 + q[2 * i + 1]; }
    const double k = (double)p.x[(long long)c * p.hw];
    const double u = a1 / p.count;
    const double mean = k + u;
    const double uu = u * u;
    double var = a2 / p.count - uu;
    if (var < 0.0) var = 0.0;
    const double ve = var + p.eps;
    p.mean[c] = (float)mean;
    p.invstd[c] = (float)(1.0 / sqrt(ve));
    if (p.runningMean) {
        const double keep = 1.0 - p.momentum;
        const double a = keep * (double)p.runningMean[c], b = p.momentum * mean;
        p.runningMean[c] = (float)(a + b);
    }
    if (p.runningVar) {
        const double keep = 1.0 - p.momentum;
        const double unbiased = var * (p.count / (p.count - 1.0));
        const double a = keep * (double)p.runningVar[c], b = p.momentum * unbiased;
        p.runningVar[c] = (float)(a + b);
    }
}

struct ApplyParams {
    const float* x; const float* residual; float* y;
    const float* mean; const float* invstd; const float* gamma; const float* beta;
    long long hw;
    int C, relu, vec;
};

// grid (chunks, C, N)
__global__ void __launch_bounds__(BN_THREADS) batch_norm_apply_kernel(const ApplyParams p)
{
    const int k = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const float mean = p.mean[c], invstd = p.invstd[c], gamma = p.gamma[c], beta = p.beta[c];
    const long long base = ((long long)n * p.C + c) * p.hw;
    const float* xp = p.x + base;
    const float* rp = p.residual ? p.residual + base : nullptr;
    float* yp = p.y + base;
    const long long lo = (long long)k * BN_CHUNK;
    const long long hi = lo + BN_CHUNK < p.hw ? lo + BN_CHUNK : p.hw;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* x4 = reinterpret_cast<const float4*>(xp + lo);
        float4* y4 = reinterpret_cast<float4*>(yp + lo);
        for (long long q = tid; q < quads; q += BN_THREADS) {
            const float4 a = x4[q];
            float4 v;
            v.x = bn_value(a.x, mean, invstd, gamma, beta, p.relu);
            v.y = bn_value(a.y, mean, invstd, gamma, beta, p.relu);
            v.z = bn_value(a.z, mean, invstd, gamma, beta, p.relu);
            v.w = bn_value(a.w, mean, invstd, gamma, beta, p.relu);
            if (rp) {
                const float4 r = reinterpret_cast<const float4*>(rp + lo)[q];
                v.x = v.x + r.x; v.y = v.y + r.y; v.z = v.z + r.z; v.w = v.w + r.w;
            }
            y4[q] = v;
        }
    } else {
        for (long long i = lo + tid; i < hi; i += BN_THREADS) {
            float v = bn_value(xp[i], mean, invstd, gamma, beta, p.relu);
            if (rp) v = v + rp[i];
            yp[i] = v;
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------

struct BnGradSumParams {
    const float* dy; const float* x; const float* y;     // y: the forward's output of the ReLU form (its sign gates dy), NULL otherwise
    const float* mean; const float* invstd;
    long long hw, chunk;
    int C, S, vec;
    double* ws;                  // [C][N S][2]
};

__device__ __forceinline__ float bn_gate(float dy, const float* y, long long i) { return y ? (y[i] > 0.0f ? dy : 0.0f) : dy; }

__global__ void __launch_bounds__(BN_THREADS) batch_norm_grad_sum_kernel(const BnGradSumParams p)
{
    __shared__ double sh[2 * BN_THREADS];
    const int s = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const float mean = p.mean[c], invstd = p.invstd[c];
    const long long base = ((long long)n * p.C + c) * p.hw;
    const float* gp = p.dy + base;
    const float* xp = p.x + base;
    const float* yp = p.y ? p.y + base : nullptr;
    const long long lo = (long long)s * p.chunk;
    const long long hi = lo + p.chunk < p.hw ? lo + p.chunk : p.hw;
    double a1 = 0.0, a2 = 0.0;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* g4 = reinterpret_cast<const float4*>(gp + lo);
        const float4* x4 = reinterpret_cast<const float4*>(xp + lo);
        for (long long q = tid; q < quads; q += BN_THREADS) {
            float4 g = g4[q];
            const float4 a = x4[q];
            if (yp) {
                const float4 o = reinterpret_cast<const float4*>(yp + lo)[q];
                g.x = o.x > 0.0f ? g.x : 0.0f; g.y = o.y > 0.0f ? g.y : 0.0f; g.z = o.z > 0.0f ? g.z : 0.0f; g.w = o.w > 0.0f ? g.w : 0.0f;
            }
            a1 = a1 + (double)g.x; a2 = fma((double)g.x, (double)bn_xhat(a.x, mean, invstd), a2);
            a1 = a1 + (double)g.y; a2 = fma((double)g.y, (double)bn_xhat(a.y, mean, invstd), a2);
            a1 = a1 + (double)g.z; a2 = fma((double)g.z, (double)bn_xhat(a.z, mean, invstd), a2);
            a1 = a1 + (double)g.w; a2 = fma((double)g.w, (double)bn_xhat(a.w, mean, invstd), a2);
        }
    } else {
        for (long long i = lo + tid; i < hi; i += BN_THREADS) {
            const float g = bn_gate(gp[i], yp, i);
            a1 = a1 + (double)g; a2 = fma((double)g, (double)bn_xhat(xp[i], mean, invstd), a2);
        }
    }
    tree_sum2(sh, a1, a2, tid);
    if (tid == 0) {
        double* o = p.ws + (((long long)c * gridDim.z + n) * p.S + s) * 2;
        o[0] = sh[0];
        o[1] = sh[BN_THREADS];
    }
}

struct GradFinishParams {
    const double* ws;
    int C, parts;
    double count;
    float* coef;                 // [C][2]: sum g / M, sum g xhat / M
    float* dgamma; float* dbeta; // NULL: not wanted
};

__global__ void __launch_bounds__(BN_THREADS) batch_norm_grad_finish_kernel(const GradFinishParams p)
{
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c >= p.C) return;
    const double* q = p.ws + (long long)c * p.parts * 2;
    double b1 = 0.0, b2 = 0.0;
    for (int i = 0; i < p.parts; ++i) { b1 = b1 + q[2 * i]; b2 = b2 + q[2 * i + 1]; }
    p.coef[2 * c] = (float)(b1 / p.count);
    p.coef[2 * c + 1] = (float)(b2 / p.count);
    if (p.dbeta) p.dbeta[c] = (float)b1;
    if (p.dgamma) p.dgamma[c] = (float)b2;
}

struct BackwardParams {
    const float* dy; const float* x; const float* y; float* dx;
    const float* mean; const float* invstd; const float* gamma; const float* coef;
    long long hw;
    int C, vec;
};

__device__ __forceinline__ float bn_dx(float g, float x, float mean, float invstd, float c1, float c2, float scale)
{
    const float a = g - c1;
    const float b = bn_xhat(x, mean, invstd) * c2;
    const float e = a - b;
    return e * scale;
}

__global__ void __launch_bounds__(BN_THREADS) batch_norm_backward_kernel(const BackwardParams p)
{
    const int k = blockIdx.x, c = blockIdx.y, n = blockIdx.z, tid = threadIdx.x;
    const float mean = p.mean[c], invstd = p.invstd[c], c1 = p.coef[2 * c], c2 = p.coef[2 * c + 1];
    const float scale = p.gamma[c] * invstd;
    const long long base = ((long long)n * p.C + c) * p.hw;
    const float* gp = p.dy + base;
    const float* xp = p.x + base;
    const float* yp = p.y ? p.y + base : nullptr;
    float* dp = p.dx + base;
    const long long lo = (long long)k * BN_CHUNK;
    const long long hi = lo + BN_CHUNK < p.hw ? lo + BN_CHUNK : p.hw;
    if (p.vec) {
        const long long quads = hi > lo ? (hi - lo) / 4 : 0;
        const float4* g4 = reinterpret_cast<const float4*>(gp + lo);
        const float4* x4 = reinterpret_cast<const float4*>(xp + lo);
        float4* d4 = reinterpret_cast<float4*>(dp + lo);
        for (long long q = tid; q < quads; q += BN_THREADS) {
            float4 g = g4[q];
            const float4 a = x4[q];
            if (yp) {
                const float4 o = reinterpret_cast<const float4*>(yp + lo)[q];
                g.x = o.x > 0.0f ? g.x : 0.0f; g.y = o.y > 0.0f ? g.y : 0.0f; g.z = o.z > 0.0f ? g.z : 0.0f; g.w = o.w > 0.0f ? g.w : 0.0f;
            }
            float4 v;
            v.x = bn_dx(g.x, a.x, mean, invstd, c1, c2, scale);
            v.y = bn_dx(g.y, a.y, mean, invstd, c1, c2, scale);
            v.z = bn_dx(g.z, a.z, mean, invstd, c1, c2, scale);
            v.w = bn_dx(g.w, a.w, mean, invstd, c1, c2, scale);
            d4[q] = v;
        }
    } else {
        for (long long i = lo + tid; i < hi; i += BN_THREADS)
            dp[i] = bn_dx(bn_gate(gp[i], yp, i), xp[i], mean, invstd, c1, c2, scale);
    }
}

}  // namespace

extern "C" {

int isrBatchNormSupported(int N, int C, int H, int W) { return bn_supported(N, C, H, W) ? 1 : 0; }

int isrBatchNormSlabs(int N, int C, int H, int W)
{
    if (!bn_supported(N, C, H, W)) return -1;
    return bn_slabs(N, C, H, W);
}

int isrBatchNormStats(const float* x, int N, int C, int H, int W, int S, double* workspace, double eps, double momentum, float* mean,
                      float* invstd, float* runningMean, float* runningVar, void* stream)
{
    if (!x || !workspace || !mean || !invstd) return -1;
    if (!bn_supported(N, C, H, W)) return -3;
    if (S != bn_slabs(N, C, H, W)) return -1;
    StatParams p;
    p.x = x; p.hw = (long long)H * W; p.chunk = bn_chunk(p.hw, S); p.C = C; p.S = S;
    p.vec = (aligned16(x) && (p.hw & 3) == 0) ? 1 : 0;
    p.ws = workspace;
    int rc = isr_launch(ISR_VARIANT_BN_STAT, 0.0, batch_norm_stat_kernel, dim3((unsigned)S, (unsigned)C, (unsigned)N), dim3(BN_THREADS), 0,
                        (hipStream_t)stream, p);
    if (rc != 0) return rc;
    StatFinishParams f;
    f.x = x; f.ws = workspace; f.hw = p.hw; f.C = C; f.parts = N * S;
    f.count = (double)N * (double)p.hw; f.eps = eps; f.momentum = momentum;
    f.mean = mean; f.invstd = invstd; f.runningMean = runningMean; f.runningVar = runningVar;
    return isr_launch(ISR_VARIANT_BN_FINISH, 0.0, batch_norm_finish_kernel, dim3((unsigned)((C + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0,
                      (hipStream_t)stream, f);
}

int isrBatchNormApply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* residual,
                      int relu, float* y, int N, int C, int H, int W, void* stream)
{
    if (!x || !mean || !invstd || !gamma || !beta || !y) return -1;
    if (!bn_supported(N, C, H, W)) return -3;
    ApplyParams p;
    p.x = x; p.residual = residual; p.y = y; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.beta = beta;
    p.hw = (long long)H * W; p.C = C; p.relu = relu ? 1 : 0;
    p.vec = (aligned16(x) && aligned16(y) && (!residual || aligned16(residual)) && (p.hw & 3) == 0) ? 1 : 0;
    const long long chunks = (p.hw + BN_CHUNK - 1) / BN_CHUNK;
    return isr_launch(ISR_VARIANT_BN_APPLY, 0.0, batch_norm_apply_kernel, dim3((unsigned)chunks, (unsigned)C, (unsigned)N), dim3(BN_THREADS), 0,
                      (hipStream_t)stream, p);
}

int isrBatchNormGradSums(const float* dy, const float* x, const float* y, const float* mean, const float* invstd, int N, int C, int H, int W,
                         int S, double* workspace, float* coef, float* dGamma, float* dBeta, void* stream)
{
    if (!dy || !x || !mean || !invstd || !workspace || !coef) return -1;
    if (!bn_supported(N, C, H, W)) return -3;
    if (S != bn_slabs(N, C, H, W)) return -1;
    BnGradSumParams p;
    p.dy = dy; p.x = x; p.y = y; p.mean = mean; p.invstd = invstd;
    p.hw = (long long)H * W; p.chunk = bn_chunk(p.hw, S); p.C = C; p.S = S;
    p.vec = (aligned16(dy) && aligned16(x) && (!y || aligned16(y)) && (p.hw & 3) == 0) ? 1 : 0;
    p.ws = workspace;
    int rc = isr_launch(ISR_VARIANT_BN_GRAD_SUM, 0.0, batch_norm_grad_sum_kernel, dim3((unsigned)S, (unsigned)C, (unsigned)N), dim3(BN_THREADS), 0,
                        (hipStream_t)stream, p);
    if (rc != 0) return rc;
    GradFinishParams f;
    f.ws = workspace; f.C = C; f.parts = N * S; f.count = (double)N * (double)p.hw;
    f.coef = coef; f.dgamma = dGamma; f.dbeta = dBeta;
    return isr_launch(ISR_VARIANT_BN_GRAD_FINISH, 0.0, batch_norm_grad_finish_kernel, dim3((unsigned)((C + BN_THREADS - 1) / BN_THREADS)),
                      dim3(BN_THREADS), 0, (hipStream_t)stream, f);
}

int isrBatchNormBackward(const float* dy, const float* x, const float* y, const float* mean, const float* invstd, const float* gamma,
                         const float* coef, float* dx, int N, int C, int H, int W, void* stream)
{
    if (!dy || !x || !mean || !invstd || !gamma || !coef || !dx) return -1;
    if (!bn_supported(N, C, H, W)) return -3;
    BackwardParams p;
    p.dy = dy; p.x = x; p.y = y; p.dx = dx; p.mean = mean; p.invstd = invstd; p.gamma = gamma; p.coef = coef;
    p.hw = (long long)H * W; p.C = C;
    p.vec = (aligned16(dy) && aligned16(x) && aligned16(dx) && (!y || aligned16(y)) && (p.hw & 3) == 0) ? 1 : 0;
    const long long chunks = (p.hw + BN_CHUNK - 1) / BN_CHUNK;
    return isr_launch(ISR_VARIANT_BN_BACKWARD, 0.0, batch_norm_backward_kernel, dim3((unsigned)chunks, (unsigned)C, (unsigned)N), dim3(BN_THREADS), 0,
                      (hipStream_t)stream, p);
}

}  // extern "C"
