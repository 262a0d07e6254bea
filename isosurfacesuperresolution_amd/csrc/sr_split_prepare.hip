// WEIGHT IMAGES of the split-operand kernels (plain, upsampling, trunk, block, transposed convolution and its data gradient): the format
// and the two kernels that write it.  (The fused tail has an operand order of its own -- tail_prepare_kernel, sr_conv_tail.hip -- and
// shares the scale rule only; the fp16 / bf16 images of sr_conv_f16.hip have no scale.)
//
// An image multiplies activations by a matrix [rows][k] per tap (rows: what the consumer produces, k: what it sums over):
//     unit 0                                              header { 2^S, 2^-S, S, 0 }: max |w| 2^S in [2^13, 2^14) (sr_split_scale.h)
//     unit 1 + (((tap ksteps + s) 2 + part) 2 + h) rowPad + row     element e = fp16 part (0 hi, 1 lo) of w 2^S at k = 16 s + 8 h + e
//     behind those, plain convolutions only: the third plane
//     unit 1 + 9 ksteps 4 rowPad + ((tap ksteps + s) 2 + h) rowPad + row     hi 2^-11, the partner of the activations' scaled low part
// with ksteps = ceil(k / 16), rowPad = rows rounded up to 32, zeros beyond rows and k.  Which source element that is:
//     image                          rows / k       element                              third plane
//     convolution, forward           Cout / Cin     w[(row Cin + k) 9 + tap]             yes
//     convolution, data gradient     Cin / Cout     w[(k Cin + row) 9 + 8 - tap]         yes
//     transposed conv., forward      co / ci        w[(k 64 + row) 9 + tap]              no
//     transposed conv., data grad.   ci / co        w[(row 64 + k) 9 + tap]              no
// i.e. per image: which dimension of the stored [d0][d1][3][3] tensor is the row, whether the taps are flipped, and whether the third
// plane is written.  Training re-prepares every layer's two images after every optimizer step: up to PM_MAX layers cost two launches.
#include "sr_split_common.h"
#include "sr_split_scale.h"

namespace {

constexpr int PM_MAX = 32;
struct ImageKind { int rowDim, flip, third; };         // rowDim: 0 = rows are d0, 1 = rows are d1
constexpr ImageKind CONV_FORWARD = {0, 0, 1}, CONV_DGRAD = {1, 1, 1}, CONVT_FORWARD = {1, 0, 0}, CONVT_DGRAD = {0, 0, 0};
constexpr int CT_C = 64;                                // the transposed convolution's channels, in and out

struct PrepParams {
    const float* w[PM_MAX];      // layer l: [d0][d1][3][3]
    u32x4* image[2][PM_MAX];     // its images of kind[0] and kind[1] (either may be NULL)
    int d0[PM_MAX], d1[PM_MAX];
    ImageKind kind[2];
};

__host__ __device__ inline int image_units(int rows, int k) { return 9 * ((k + 15) / 16) * 2 * (((rows + 31) / 32) * 32); }   // (tap, k-step, half, row)

// hi 2^-11, element-wise in fp16 (IEEE, subnormals kept): the value `a0h * (_Float16)0.00048828125f` has in the kernels
__device__ __forceinline__ f16x8 split_scaled_hi(f16x8 qh) { return qh * (_Float16)0.00048828125f; }

// one workgroup per layer, wide and with independent loads in flight: the header of both images (the same numbers: the same scale)
__global__ __launch_bounds__(1024) void split_scale_kernel(const PrepParams p)
{
    const int l = blockIdx.x;
    const float* __restrict__ w = p.w[l];
    const int count = p.d0[l] * p.d1[l] * 9;
    float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f;
    int i = threadIdx.x;
    for (; i + 3072 < count; i += 4096) {
        m0 = isr_max(m0, fabsf(w[i])); m1 = isr_max(m1, fabsf(w[i + 1024]));
        m2 = isr_max(m2, fabsf(w[i + 2048])); m3 = isr_max(m3, fabsf(w[i + 3072]));
    }
    for (; i < count; i += 1024) m0 = isr_max(m0, fabsf(w[i]));
    const float mx = isr_block_max(isr_max(isr_max(m0, m1), isr_max(m2, m3)));
    if (threadIdx.x == 0) {
        const int S = isr_scale_exponent(mx);
        if (p.image[0][l]) isr_scale_header(S, p.image[0][l]);
        if (p.image[1][l]) isr_scale_header(S, p.image[1][l]);
    }
}

// grid: (units, 2 n): blockIdx.y = 2 layer + which image
__global__ __launch_bounds__(256) void split_layout_kernel(const PrepParams p)
{
    const int l = blockIdx.y >> 1;
    const ImageKind kind = p.kind[blockIdx.y & 1];
    u32x4* __restrict__ wq = p.image[blockIdx.y & 1][l];
    if (!wq) return;
    const float* __restrict__ w = p.w[l];
    const int d1 = p.d1[l];
    const int rows = kind.rowDim ? d1 : p.d0[l], K = kind.rowDim ? p.d0[l] : d1;
    const int rowStride = kind.rowDim ? 1 : d1, kStride = kind.rowDim ? d1 : 1;
    const int ksteps = (K + 15) / 16, rowPad = ((rows + 31) / 32) * 32;
    const float scale = reinterpret_cast<const float*>(wq)[0];
    const int total = image_units(rows, K);
    for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < total; u += gridDim.x * blockDim.x) {
        const int row = u % rowPad;
        const int hh = (u / rowPad) & 1;
        const int s = (u / (rowPad * 2)) % ksteps;
        const int tap = u / (rowPad * 2 * ksteps);
        f16x8 qh, ql;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 16 * s + 8 * hh + e;
            float v = 0.0f;
            if (row < rows && k < K) v = w[((size_t)row * rowStride + (size_t)k * kStride) * 9 + (kind.flip ? 8 - tap : tap)];
            _Float16 a, b;
            split16(v * scale, a, b);
            qh[e] = a; ql[e] = b;
        }
        const size_t base = 1 + (size_t)(((tap * ksteps + s) * 2 + 0) * 2 + hh) * rowPad + row;
        wq[base] = __builtin_bit_cast(u32x4, qh);
        wq[base + (size_t)2 * rowPad] = __builtin_bit_cast(u32x4, ql);
        if (kind.third)
            wq[1 + (size_t)9 * ksteps * 4 * rowPad + (size_t)((tap * ksteps + s) * 2 + hh) * rowPad + row] = __builtin_bit_cast(u32x4, split_scaled_hi(qh));
    }
}

// n layers, per layer the images a[l] of kind ka and b[l] of kind kb (a or b may be NULL, and so may either image of a layer -- not both)
int prepare_images(int n, const float* const* w, void* const* a, void* const* b, const int* d0, const int* d1, ImageKind ka, ImageKind kb, void* stream)
{
    if (n <= 0 || n > PM_MAX || !w || !d0 || !d1 || (!a && !b)) return -1;
    PrepParams p;
    p.kind[0] = ka; p.kind[1] = kb;
    int most = 0;
    for (int l = 0; l < PM_MAX; ++l) {
        const bool on = l < n;
        p.w[l] = on ? w[l] : nullptr;
        p.image[0][l] = on && a ? (u32x4*)a[l] : nullptr;
        p.image[1][l] = on && b ? (u32x4*)b[l] : nullptr;
        p.d0[l] = on ? d0[l] : 0; p.d1[l] = on ? d1[l] : 0;
        if (on) {
            if (!w[l] || d0[l] <= 0 || d1[l] <= 0 || (!p.image[0][l] && !p.image[1][l])) return -1;
            const int u0 = image_units(d0[l], d1[l]), u1 = image_units(d1[l], d0[l]);
            most = u0 > most ? u0 : most; most = u1 > most ? u1 : most;
        }
    }
    hipLaunchKernelGGL(split_scale_kernel, dim3(n), dim3(1024), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(split_layout_kernel, dim3((most + 255) / 256, 2 * n), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

long long image_bytes(int rows, int k, bool third) { return 16 + (long long)image_units(rows, k) * (third ? 3 : 2) * 16; }

} // namespace

extern "C" {

long long isrConvSplitWeightBytes(int Cin, int Cout)
{
    if (Cin <= 0 || Cout <= 0) return -1;
    return image_bytes(Cout, Cin, true);
}

int isrConvSplitPrepare(const float* w, void* wq, int Cout, int Cin, void* stream)
{
    if (!w || !wq) return -1;
    return prepare_images(1, &w, &wq, nullptr, &Cout, &Cin, CONV_FORWARD, CONV_DGRAD, stream);
}

int isrConvSplitPrepareManyMax(void) { return PM_MAX; }

int isrConvSplitPrepareMany(int n, const float* const* w, void* const* wqForward, void* const* wqBackward, const int* cout, const int* cin, void* stream)
{
    return prepare_images(n, w, wqForward, wqBackward, cout, cin, CONV_FORWARD, CONV_DGRAD, stream);
}

long long isrConvTransposeSplitWeightBytes(void) { return image_bytes(CT_C, CT_C, false); }

int isrConvTransposeSplitPrepare(const float* w, void* wq, void* stream)
{
    if (!w || !wq) return -1;
    return prepare_images(1, &w, &wq, nullptr, &CT_C, &CT_C, CONVT_FORWARD, CONVT_DGRAD, stream);
}

long long isrConvTransposeDataGradWeightBytes(void) { return image_bytes(CT_C, CT_C, false); }

int isrConvTransposeDataGradPrepare(const float* w, void* wq, void* stream)
{
    if (!w || !wq) return -1;
    return prepare_images(1, &w, nullptr, &wq, &CT_C, &CT_C, CONVT_FORWARD, CONVT_DGRAD, stream);
}

} // extern "C"
