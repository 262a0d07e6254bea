// The metric stage of the statistics harness (include/isr_sr_kernels.h: isrMetrics*): masked squared error, the ten MS-SSIM terms and
// the absolute-difference histogram of an image pair -- what stats.Statistics evaluates per frame with fp64 torch operations
// (utils/psnr.py, utils/ssim.py, np.histogram) -- as kernels that read the fp32 frames where they lie (cropped views: pitches).
//
// DEFINED by that Python code evaluated in fp64: every value is widened on load and every operation below is the fp64 operation of the
// definition, in its order, with no contraction into FMAs (file-scope pragma).  What is NOT fixed by the definition is the order of the
// sums (the 121 taps of a window, the mean over an image): here they are
//   per thread   : in index order,
//   per workgroup: an LDS tree in a fixed shape,
//   per image    : the workgroups' partial sums, summed by ONE workgroup in the same two steps,
// so a result depends on the shapes only -- no floating-point atomics, two calls give the same bits.  The histogram counts with integer
// atomics (LDS, then global), which commute.
//
// MS-SSIM is a chain of launches on one stream, nothing read back in between:
//   minmax(level 0) ; for each level: ssim(level) , pool(level -> level + 1, with the min / max of its output) ; combine
// The SSIM launch of a level reduces the min / max partials of that level itself (at most kPartials pairs) to pick C1 / C2.  Level 0 is
// read from the fp32 frames (blended on load), levels 1 .. 4 are fp64 planes in the workspace (1/3 of the frame).
// SSIM tile: 32 x 8 outputs per workgroup, one per thread; both images' (8 + k - 1) x (32 + k - 1) fp64 tile and the k x k window in LDS
// (k = 11: 2 x 6048 + 968 bytes; with the reduction scratch 17 KB of the CU's 160 KB).
#include <hip/hip_runtime.h>
#include "../../include/isr_sr_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPartials = 1024;          // workgroups of a grid-stride reduction (squared error, min / max, pooling): partial pairs per level
constexpr int kLevels = 5;
constexpr int kWin = 11;
constexpr int kTileW = 32, kTileH = 8;
constexpr int kMaxBins = 1024;
constexpr int kMaxSize = 32768;          // H, W: pixel counts stay below 2^31

// the two images of one MS-SSIM level (or of a squared-error / histogram call: level 0)
struct Pair {
    const float* a32; const float* b32;              // level 0: fp32 frames, pitches in floats
    long long aRow, aPlane, bRow, bPlane;
    const double* blend; long long blendRow;         // level 0: a' = b + m (a - b), or NULL
    const double* a64; const double* b64;            // levels 1 .. 4: contiguous fp64 [C][H][W] (a32 == NULL)
    int C, H, W;
};

__device__ __forceinline__ void load_pair(const Pair& s, int c, int y, int x, double& a, double& b)
{
    if (s.a32) {
        a = (double)s.a32[c * s.aPlane + y * s.aRow + x];
        b = (double)s.b32[c * s.bPlane + y * s.bRow + x];
        if (s.blend) {
            const double m = s.blend[y * s.blendRow + x];
            const double d = a - b;
            a = b + m * d;
        }
    } else {
        const size_t i = ((size_t)c * s.H + y) * s.W + x;
        a = s.a64[i];
        b = s.b64[i];
    }
}

// min / max that keep a NaN (torch.min / torch.max do: the range guess then sees comparisons that are false)
__device__ __forceinline__ double nan_min(double x, double y) { return x != x ? x : (y != y ? y : (y < x ? y : x)); }
__device__ __forceinline__ double nan_max(double x, double y) { return x != x ? x : (y != y ? y : (y > x ? y : x)); }

// the workgroup's sum of v in a fixed tree; every thread gets it.  sh: kThreads doubles
__device__ __forceinline__ double block_sum(double v, double* sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ void block_minmax(double& mn, double& mx, double* sh_min, double* sh_max)
{
    const int t = threadIdx.x;
    sh_min[t] = mn;
    sh_max[t] = mx;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            sh_min[t] = nan_min(sh_min[t], sh_min[t + s]);
            sh_max[t] = nan_max(sh_max[t], sh_max[t + s]);
        }
        __syncthreads();
    }
    mn = sh_min[0];
    mx = sh_max[0];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- squared error

// partial[2 g] = the workgroup's sum of (m a - m b)^2, partial[2 g + 1] = its sum of m
__global__ void __launch_bounds__(kThreads) sq_err_kernel(const Pair s, const double* mask, long long maskRow, double* partial)
{
    __shared__ double sh[kThreads];
    const long long pixels = (long long)s.H * s.W;
    double sq = 0.0, ms = 0.0;
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < pixels; p += (long long)gridDim.x * kThreads) {
        const int y = (int)(p / s.W), x = (int)(p - (long long)y * s.W);
        const double m = mask ? mask[y * maskRow + x] : 1.0;
        ms = ms + m;
        for (int c = 0; c < s.C; ++c) {
            double a, b;
            load_pair(s, c, y, x, a, b);
            const double d = m * a - m * b;
            sq = sq + d * d;
        }
    }
    sq = block_sum(sq, sh);
    ms = block_sum(ms, sh);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sq;
        partial[2 * blockIdx.x + 1] = ms;
    }
}

// out[j] = sum over g < n of partial[2 g + j], j = 0, 1: one workgroup
__global__ void __launch_bounds__(kThreads) sum_pairs_kernel(const double* partial, int n, double* out)
{
    __shared__ double sh[kThreads];
    double s0 = 0.0, s1 = 0.0;
    for (int g = threadIdx.x; g < n; g += kThreads) {
        s0 = s0 + partial[2 * g];
        s1 = s1 + partial[2 * g + 1];
    }
    s0 = block_sum(s0, sh);
    s1 = block_sum(s1, sh);
    if (threadIdx.x == 0) {
        out[0] = s0;
        out[1] = s1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- MS-SSIM

// partial[2 g] / [2 g + 1] = min / max of image a' over the workgroup's share of the level
__global__ void __launch_bounds__(kThreads) minmax_kernel(const Pair s, double* partial)
{
    __shared__ double sh_min[kThreads], sh_max[kThreads];
    const long long pixels = (long long)s.H * s.W;
    double mn = INFINITY, mx = -INFINITY;
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < pixels; p += (long long)gridDim.x * kThreads) {
        const int y = (int)(p / s.W), x = (int)(p - (long long)y * s.W);
        for (int c = 0; c < s.C; ++c) {
            double a, b;
            load_pair(s, c, y, x, a, b);
            mn = nan_min(mn, a);
            mx = nan_max(mx, a);
        }
    }
    block_minmax(mn, mx, sh_min, sh_max);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = mn;
        partial[2 * blockIdx.x + 1] = mx;
    }
}

// avg_pool2d(2) of both images (sum of the four in row-major order, divided by 4) into contiguous fp64 planes [C][H/2][W/2], and the
// min / max partials of the pooled image a
__global__ void __launch_bounds__(kThreads) pool_kernel(const Pair s, double* a_out, double* b_out, double* partial)
{
    __shared__ double sh_min[kThreads], sh_max[kThreads];
    const int Ho = s.H / 2, Wo = s.W / 2;
    const long long pixels = (long long)Ho * Wo;
    double mn = INFINITY, mx = -INFINITY;
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < pixels; p += (long long)gridDim.x * kThreads) {
        const int y = (int)(p / Wo), x = (int)(p - (long long)y * Wo);
        for (int c = 0; c < s.C; ++c) {
            double a00, a01, a10, a11, b00, b01, b10, b11;
            load_pair(s, c, 2 * y, 2 * x, a00, b00);
            load_pair(s, c, 2 * y, 2 * x + 1, a01, b01);
            load_pair(s, c, 2 * y + 1, 2 * x, a10, b10);
            load_pair(s, c, 2 * y + 1, 2 * x + 1, a11, b11);
            const double a = (((a00 + a01) + a10) + a11) / 4.0;
            const double b = (((b00 + b01) + b10) + b11) / 4.0;
            const size_t o = (size_t)c * pixels + p;
            a_out[o] = a;
            b_out[o] = b;
            mn = nan_min(mn, a);
            mx = nan_max(mx, a);
        }
    }
    block_minmax(mn, mx, sh_min, sh_max);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = mn;
        partial[2 * blockIdx.x + 1] = mx;
    }
}

// One 32 x 8 tile of one channel's SSIM map (utils/ssim.py: ssim): partial[2 g] = the tile's sum of the map, partial[2 g + 1] = its sum
// of v1 / v2; g = the workgroup's linear index.  range_partial: the level's n_range min / max pairs.
__global__ void __launch_bounds__(kThreads) ssim_kernel(const Pair s, int k, const double* window, const double* range_partial, int n_range,
                                                        double* partial)
{
    __shared__ double sa[(kTileH + kWin - 1) * (kTileW + kWin - 1)], sb[(kTileH + kWin - 1) * (kTileW + kWin - 1)];
    __shared__ double sw[kWin * kWin];
    __shared__ double sh0[kThreads], sh1[kThreads];
    const int t = threadIdx.x;
    // the dynamic range of the level, guessed from image a' (ssim.py: _dynamic_range)
    double mn = INFINITY, mx = -INFINITY;
    for (int g = t; g < n_range; g += kThreads) {
        mn = nan_min(mn, range_partial[2 * g]);
        mx = nan_max(mx, range_partial[2 * g + 1]);
    }
    block_minmax(mn, mx, sh0, sh1);
    const double L = (mx > 128.0 ? 255.0 : 1.0) - (mn < -0.5 ? -1.0 : 0.0);
    const double c1 = 0.01 * L, c2 = 0.03 * L;
    const double C1 = c1 * c1, C2 = c2 * c2;

    const int c = blockIdx.z, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int tw = kTileW + k - 1, th = kTileH + k - 1;
    for (int i = t; i < th * tw; i += kThreads) {
        const int ly = i / tw, lx = i - ly * tw;
        double a = 0.0, b = 0.0;
        if (y0 + ly < s.H && x0 + lx < s.W) load_pair(s, c, y0 + ly, x0 + lx, a, b);
        sa[i] = a;
        sb[i] = b;
    }
    for (int i = t; i < k * k; i += kThreads) sw[i] = window[i];
    __syncthreads();

    const int Ho = s.H - k + 1, Wo = s.W - k + 1;
    const int tx = t % kTileW, ty = t / kTileW;
    double map = 0.0, cs = 0.0;
    if (x0 + tx < Wo && y0 + ty < Ho) {
        double mu1 = 0.0, mu2 = 0.0, e11 = 0.0, e22 = 0.0, e12 = 0.0;
        for (int i = 0; i < k; ++i) {
            const double* ra = sa + (ty + i) * tw + tx, * rb = sb + (ty + i) * tw + tx, * rw = sw + i * k;
            for (int j = 0; j < k; ++j) {
                const double w = rw[j], a = ra[j], b = rb[j];
                mu1 = mu1 + w * a;
                mu2 = mu2 + w * b;
                e11 = e11 + w * (a * a);
                e22 = e22 + w * (b * b);
                e12 = e12 + w * (a * b);
            }
        }
        const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const double s1 = e11 - mu1_sq, s2 = e22 - mu2_sq, s12 = e12 - mu12;
        const double v1 = 2.0 * s12 + C2;
        const double v2 = s1 + s2 + C2;
        cs = v1 / v2;
        map = ((2.0 * mu12 + C1) * v1) / ((mu1_sq + mu2_sq + C1) * v2);
    }
    map = block_sum(map, sh0);
    cs = block_sum(cs, sh0);
    if (t == 0) {
        const size_t g = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * g] = map;
        partial[2 * g + 1] = cs;
    }
}

struct CombineArgs {
    const double* partial[kLevels];      // the level's SSIM partial pairs
    int n[kLevels];                      // how many
    double count[kLevels];               // C Ho Wo of the level: the means' divisor
};

// out[0..4] = mean SSIM map per level, out[5..9] = mean v1 / v2 per level, out[10] = the MS-SSIM of utils/ssim.py:62
__global__ void __launch_bounds__(kThreads) combine_kernel(const CombineArgs q, double* out)
{
    __shared__ double sh[kThreads];
    __shared__ double terms[2 * kLevels];
    for (int l = 0; l < kLevels; ++l) {
        double s0 = 0.0, s1 = 0.0;
        for (int g = threadIdx.x; g < q.n[l]; g += kThreads) {
            s0 = s0 + q.partial[l][2 * g];
            s1 = s1 + q.partial[l][2 * g + 1];
        }
        s0 = block_sum(s0, sh);
        s1 = block_sum(s1, sh);
        if (threadIdx.x == 0) {
            terms[l] = s0 / q.count[l];
            terms[kLevels + l] = s1 / q.count[l];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double w[kLevels] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        // prod((css ** w)[:-1] * (sims ** w)[-1]): the last level's SSIM power multiplies each of the four factors
        const double last = pow(terms[kLevels - 1], w[kLevels - 1]);
        double prod = 1.0;
        for (int l = 0; l < kLevels - 1; ++l) {
            const double f = pow(terms[kLevels + l], w[l]) * last;
            prod = l == 0 ? f : prod * f;
        }
        for (int i = 0; i < 2 * kLevels; ++i) out[i] = terms[i];
        out[2 * kLevels] = prod;
    }
}

// -------------------------------------------------------------------------------------------------------------------- histogram

__global__ void __launch_bounds__(kThreads) histogram_kernel(const Pair s, double scale, int bins, const double* edges,
                                                             unsigned long long* counts)
{
    __shared__ unsigned int local[kMaxBins + 1];
    for (int i = threadIdx.x; i <= bins; i += kThreads) local[i] = 0u;
    __syncthreads();
    const long long pixels = (long long)s.H * s.W;
    unsigned int inside = 0u;
    for (long long p = (long long)blockIdx.x * kThreads + threadIdx.x; p < pixels; p += (long long)gridDim.x * kThreads) {
        const int y = (int)(p / s.W), x = (int)(p - (long long)y * s.W);
        double sum = 0.0;
        for (int c = 0; c < s.C; ++c) {
            double a, b;
            load_pair(s, c, y, x, a, b);
            const double d = fabs(a - b);
            sum = c == 0 ? d : sum + d;
        }
        const double v = scale * sum;
        if (!(v >= 0.0 && v <= 1.0)) continue;                  // outside the range (or NaN): dropped
        int i = (int)(v * (double)bins);
        if (i == bins) i = bins - 1;                            // 1.0 belongs to the last bin
        if (v < edges[i]) i = i - 1;                            // (np.histogram: the product may have rounded across an edge)
        else if (v >= edges[i + 1] && i != bins - 1) i = i + 1;
        atomicAdd(&local[i], 1u);
        inside = inside + 1u;
    }
    if (inside) atomicAdd(&local[bins], inside);
    __syncthreads();
    for (int i = threadIdx.x; i <= bins; i += kThreads)
        if (local[i]) atomicAdd(&counts[i], (unsigned long long)local[i]);
}

// ------------------------------------------------------------------------------------------------------------------------- host

bool make_pair(Pair& s, const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
               const double* blend, long long blendRow, int C, int H, int W)
{
    if (!a || !b || C < 1 || C > 64 || H < 1 || W < 1 || H > kMaxSize || W > kMaxSize) return false;
    if (aRow < W || bRow < W || aPlane < 0 || bPlane < 0) return false;
    if (C > 1 && (aPlane < 1 || bPlane < 1)) return false;
    if (blend && blendRow < W) return false;
    s = Pair{a, b, aRow, aPlane, bRow, bPlane, blend, blendRow, nullptr, nullptr, C, H, W};
    return true;
}

int stride_grid(long long pixels)
{
    const long long g = (pixels + kThreads - 1) / kThreads;
    return (int)(g < 1 ? 1 : (g > kPartials ? kPartials : g));
}

int window_of(int H, int W) { return H < kWin ? (H < W ? H : W) : (W < kWin ? W : kWin); }

long long ssim_tiles(int C, int H, int W)
{
    const int k = window_of(H, W);
    const long long tx = (W - k + 1 + kTileW - 1) / kTileW, ty = (H - k + 1 + kTileH - 1) / kTileH;
    return tx * ty * C;
}

// workspace, in doubles: [kLevels][2 kPartials] min / max pairs | per level 2 ssim_tiles | per level 1 .. 4 the planes of a, of b
struct Layout {
    long long range[kLevels], ssim[kLevels], a[kLevels], b[kLevels], total;
    int H[kLevels], W[kLevels];
};

Layout layout_of(int C, int H, int W)
{
    Layout L;
    long long at = 0;
    for (int l = 0; l < kLevels; ++l) {
        L.H[l] = H >> l;
        L.W[l] = W >> l;
        L.range[l] = at;
        at += 2 * kPartials;
    }
    for (int l = 0; l < kLevels; ++l) {
        L.ssim[l] = at;
        at += 2 * ssim_tiles(C, L.H[l], L.W[l]);
    }
    L.a[0] = L.b[0] = 0;
    for (int l = 1; l < kLevels; ++l) {
        const long long n = (long long)C * L.H[l] * L.W[l];
        L.a[l] = at;
        L.b[l] = at + n;
        at += 2 * n;
    }
    L.total = at;
    return L;
}

}  // namespace

extern "C" {

int isrMetricsSqErr(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                    const double* mask, long long maskRow, int C, int H, int W, void* workspace, double* out, void* stream)
{
    Pair s;
    if (!make_pair(s, a, aRow, aPlane, b, bRow, bPlane, nullptr, 0, C, H, W) || !workspace || !out) return -1;
    if (mask && maskRow < W) return -1;
    static_assert(2 * kPartials * sizeof(double) == ISR_METRICS_SQERR_WORKSPACE_BYTES, "the header's workspace size");
    const int grid = stride_grid((long long)H * W);
    double* partial = (double*)workspace;
    hipLaunchKernelGGL(sq_err_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, s, mask, maskRow, partial);
    hipLaunchKernelGGL(sum_pairs_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, partial, grid, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

long long isrMetricsMsssimWorkspace(int C, int H, int W)
{
    if (C < 1 || C > 64 || H < 32 || W < 32 || H > kMaxSize || W > kMaxSize) return -1;
    return layout_of(C, H, W).total * (long long)sizeof(double);
}

int isrMetricsMsssim(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                     const double* blend, long long blendRow, int C, int H, int W, const double* windows, void* workspace, double* out,
                     void* stream)
{
    Pair s;
    if (!make_pair(s, a, aRow, aPlane, b, bRow, bPlane, blend, blendRow, C, H, W) || !windows || !workspace || !out) return -1;
    if (H < 32 || W < 32) return -1;                                 // (five levels, each pooled: utils/ssim.py pools the fifth as well)
    const Layout L = layout_of(C, H, W);
    double* ws = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    CombineArgs q;
    int n_range = stride_grid((long long)H * W);
    hipLaunchKernelGGL(minmax_kernel, dim3(n_range), dim3(kThreads), 0, st, s, ws + L.range[0]);
    for (int l = 0; l < kLevels; ++l) {
        const int k = window_of(s.H, s.W);
        const int Ho = s.H - k + 1, Wo = s.W - k + 1;
        const dim3 grid((Wo + kTileW - 1) / kTileW, (Ho + kTileH - 1) / kTileH, C);
        hipLaunchKernelGGL(ssim_kernel, grid, dim3(kThreads), 0, st, s, k, windows + (size_t)l * kWin * kWin, ws + L.range[l], n_range,
                           ws + L.ssim[l]);
        q.partial[l] = ws + L.ssim[l];
        q.n[l] = (int)(grid.x * grid.y * grid.z);
        q.count[l] = (double)C * (double)Ho * (double)Wo;
        if (l + 1 < kLevels) {
            n_range = stride_grid((long long)L.H[l + 1] * L.W[l + 1]);
            hipLaunchKernelGGL(pool_kernel, dim3(n_range), dim3(kThreads), 0, st, s, ws + L.a[l + 1], ws + L.b[l + 1], ws + L.range[l + 1]);
            s = Pair{nullptr, nullptr, 0, 0, 0, 0, nullptr, 0, ws + L.a[l + 1], ws + L.b[l + 1], C, L.H[l + 1], L.W[l + 1]};
        }
    }
    hipLaunchKernelGGL(combine_kernel, dim3(1), dim3(kThreads), 0, st, q, out);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int isrMetricsAbsDiffHistogram(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                               const double* blend, long long blendRow, int C, int H, int W, double scale, int bins, const double* edges,
                               long long* counts, void* stream)
{
    Pair s;
    if (!make_pair(s, a, aRow, aPlane, b, bRow, bPlane, blend, blendRow, C, H, W) || !edges || !counts) return -1;
    if (bins < 1 || bins > kMaxBins) return -1;
    if (hipMemsetAsync(counts, 0, (size_t)(bins + 1) * sizeof(long long), (hipStream_t)stream) != hipSuccess) return -2;
    hipLaunchKernelGGL(histogram_kernel, dim3(stride_grid((long long)H * W)), dim3(kThreads), 0, (hipStream_t)stream, s, scale, bins, edges,
                       (unsigned long long*)counts);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
