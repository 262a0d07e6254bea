// Device-resident training clips (dataset_video.DeviceClips; include/isr_sr_kernels.h: isrClipGather): ONE launch turns a vector of
// sample indices into the three tensors of a training batch -- input [B][T][Cl][c][c], flow [B][T][2][c][c], target [B][T][Ch][r c][r c],
// packed fp32 -- from clips that live on the device, i.e. what DatasetFromSamples.__getitem__ + data_augmentation + the default collate
// do on the host.  Pure data movement: a value is copied, or copied with its sign bit flipped (0.0 becomes -0.0, as numpy's negation
// gives), so the result equals the host path's bit for bit.
//
//   clip_gather_kernel<VEC>   grid (x, B): the workgroups of row blockIdx.y write batch element b = blockIdx.y and stride over its
//                             work items: first the high-resolution part (93 % of the bytes at r = 4), then low, then flow.
//     high, VEC       : one item = four consecutive floats of one output row, one 16-byte load and one 16-byte store.  A row of the
//                       high-resolution crop starts at column r y0 of a row of r W floats behind an offset that is a multiple of four:
//                       with r a multiple of four every quad is 16-byte aligned.  A column flip mirrors the quad's position in the row
//                       and reverses its four components.
//     high, otherwise : one item = one float (r not a multiple of four, or a buffer that is not 16-byte aligned).
//     low, flow       : one item = one float -- a crop row starts at any column.  The per-flip sign masks say which channels a row flip
//                       (mode bit 0) and a column flip (mode bit 1) negate; the kernel knows nothing about channel layouts.
//
// Addressing: an item's position INSIDE batch element b is a 32-bit number (the launcher refuses a batch element of 2^31 items or more);
// every offset into a flat clip buffer or an output tensor is a 64-bit element count -- a flat high-resolution buffer passes 2^31 elements
// at the reference's dataset size.  A batch index is clamped to [0, samples - 1]: whatever the index vector holds, the kernel reads
// table rows that exist; the tables themselves (offsets, crop boxes inside their clips) are validated where they are built, on the host.
// No LDS, no atomics, no waiting on other workgroups; plain pointer loads and stores.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/isr_sr_kernels.h"
#include "sr_profile.h"

namespace {

constexpr int CG_THREADS = 256;
constexpr int CG_MAX_GROUPS = 2048;              // eight workgroups per CU of an MI355X; the rest is strided over
constexpr int CG_CLIP_WORDS = 5;                 // clip table row: high offset, low offset, flow offset, low-res height, low-res width
constexpr int CG_SAMPLE_WORDS = 4;               // sample table row: clip, first row x0, first column y0, augmentation mode
constexpr int ISR_VARIANT_CLIP_GATHER = 60;      // ops.VARIANT_NAMES

struct ClipGatherParams {
    const float* high; const float* low; const float* flow;
    const long long* clips;          // [clips][CG_CLIP_WORDS]
    const int* samples;              // [samples][CG_SAMPLE_WORDS]
    const long long* indices;        // [B]
    float* input; float* flowOut; float* target;
    long long numSamples;
    int T, Cl, Ch, c, r, augment;
    unsigned lowNegX, lowNegY, flowNegX, flowNegY;       // bit ch: the flip negates channel ch
};

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// items of one batch element, or -1 where the shape is not one the kernel takes
long long cg_items(int B, int T, int Cl, int Ch, int c, int r, bool vec)
{
    if (B <= 0 || B > 65535 || T <= 0 || Cl <= 0 || Cl > 32 || Ch <= 0 || Ch > 32 || c <= 0 || r <= 0) return -1;
    if (c > 32768 || r > 32768 || (long long)c * r > 32768) return -1;
    const long long hr = (long long)c * r;
    const long long nh = (long long)T * Ch * hr * hr, nl = (long long)T * Cl * c * c, nf = (long long)T * 2 * c * c;
    if (nh >= (1ll << 31) || nl >= (1ll << 31) || nf >= (1ll << 31)) return -1;
    return (vec ? nh / 4 : nh) + nl + nf;
}

__device__ __forceinline__ float flip_sign(float v, unsigned on)
{
    return __uint_as_float(__float_as_uint(v) ^ (on << 31));
}

// One [T][C][n][n] crop of a [T][C][H][W] clip at (x0, y0), flipped as (fx, fy) say, float by float; item e of the packed output.
__device__ __forceinline__ void gather_floats(const float* __restrict__ src, float* __restrict__ dst, unsigned items, int C, int n,
                                              long long H, long long W, long long x0, long long y0, unsigned fx, unsigned fy,
                                              unsigned negX, unsigned negY, unsigned first, unsigned stride)
{
    const unsigned un = (unsigned)n, uC = (unsigned)C;
    for (unsigned e = first; e < items; e += stride) {
        const unsigned col = e % un, rest = e / un;
        const unsigned row = rest % un, plane = rest / un;           // plane = t C + ch
        const unsigned ch = plane % uC;
        const unsigned srow = fx ? un - 1 - row : row, scol = fy ? un - 1 - col : col;
        float v = src[((long long)plane * H + x0 + srow) * W + y0 + scol];
        v = flip_sign(v, fx & (negX >> ch) & 1u);
        v = flip_sign(v, fy & (negY >> ch) & 1u);
        dst[e] = v;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(CG_THREADS) clip_gather_kernel(const ClipGatherParams p)
{
    const int b = blockIdx.y;
    long long s = p.indices[b];
    s = s < 0 ? 0 : (s > p.numSamples - 1 ? p.numSamples - 1 : s);
    const int* sample = p.samples + s * CG_SAMPLE_WORDS;
    const long long* clip = p.clips + (long long)sample[0] * CG_CLIP_WORDS;
    const long long x0 = sample[1], y0 = sample[2];
    const unsigned mode = p.augment ? (unsigned)sample[3] : 0u;
    const unsigned fx = mode & 1u, fy = (mode >> 1) & 1u;
    const long long H = clip[3], W = clip[4];
    const unsigned first = blockIdx.x * CG_THREADS + threadIdx.x, stride = gridDim.x * CG_THREADS;
    const long long r = p.r;
    const int hr = p.c * p.r;                                        // side of the high-resolution crop

    const float* high = p.high + clip[0];
    float* target = p.target + (long long)b * p.T * p.Ch * hr * hr;
    if (VEC) {
        const unsigned qw = (unsigned)hr / 4u, uhr = (unsigned)hr;
        const unsigned quads = (unsigned)p.T * (unsigned)p.Ch * uhr * qw;
        const long long Wh = r * W, Hh = r * H;
        float4* out4 = reinterpret_cast<float4*>(target);
        for (unsigned q = first; q < quads; q += stride) {
            const unsigned qx = q % qw, rest = q / qw;
            const unsigned row = rest % uhr, plane = rest / uhr;     // plane = t Ch + ch
            const unsigned srow = fx ? uhr - 1 - row : row, sqx = fy ? qw - 1 - qx : qx;
            const float4 a = *reinterpret_cast<const float4*>(high + ((long long)plane * Hh + r * x0 + srow) * Wh + r * y0 + 4ll * sqx);
            float4 v;
            v.x = fy ? a.w : a.x; v.y = fy ? a.z : a.y; v.z = fy ? a.y : a.z; v.w = fy ? a.x : a.w;
            out4[q] = v;
        }
    } else {
        gather_floats(high, target, (unsigned)p.T * (unsigned)p.Ch * (unsigned)hr * (unsigned)hr, p.Ch, hr, r * H, r * W, r * x0, r * y0,
                      fx, fy, 0u, 0u, first, stride);
    }
    const unsigned cc = (unsigned)p.c * (unsigned)p.c;
    gather_floats(p.low + clip[1], p.input + (long long)b * p.T * p.Cl * cc, (unsigned)p.T * (unsigned)p.Cl * cc, p.Cl, p.c, H, W, x0, y0,
                  fx, fy, p.lowNegX, p.lowNegY, first, stride);
    gather_floats(p.flow + clip[2], p.flowOut + (long long)b * p.T * 2 * cc, (unsigned)p.T * 2u * cc, 2, p.c, H, W, x0, y0,
                  fx, fy, p.flowNegX, p.flowNegY, first, stride);
}

}  // namespace

extern "C" {

int isrClipGatherSupported(int B, int T, int Cl, int Ch, int c, int r) { return cg_items(B, T, Cl, Ch, c, r, false) > 0 ? 1 : 0; }

int isrClipGather(const float* high, const float* low, const float* flow, const long long* clipTable, const int* sampleTable,
                  long long numSamples, const long long* indices, int B, int T, int Cl, int Ch, int c, int r, int augment,
                  unsigned lowNegX, unsigned lowNegY, unsigned flowNegX, unsigned flowNegY, int highQuadAligned,
                  float* input, float* flowOut, float* target, void* stream)
{
    if (!high || !low || !flow || !clipTable || !sampleTable || !indices || !input || !flowOut || !target || numSamples <= 0) return -1;
    const bool vec = highQuadAligned && (r & 3) == 0 && aligned16(high) && aligned16(target);
    const long long items = cg_items(B, T, Cl, Ch, c, r, vec);
    if (items <= 0) return -3;
    ClipGatherParams p;
    p.high = high; p.low = low; p.flow = flow; p.clips = clipTable; p.samples = sampleTable; p.indices = indices;
    p.input = input; p.flowOut = flowOut; p.target = target;
    p.numSamples = numSamples;
    p.T = T; p.Cl = Cl; p.Ch = Ch; p.c = c; p.r = r; p.augment = augment ? 1 : 0;
    p.lowNegX = lowNegX; p.lowNegY = lowNegY; p.flowNegX = flowNegX; p.flowNegY = flowNegY;
    // one row of workgroups per batch element, enough for one item per thread, CG_MAX_GROUPS in all
    long long groups = (items + CG_THREADS - 1) / CG_THREADS;
    const long long most = CG_MAX_GROUPS / B > 1 ? CG_MAX_GROUPS / B : 1;
    if (groups > most) groups = most;
    const dim3 grid((unsigned)groups, (unsigned)B);
    if (vec) return isr_launch(ISR_VARIANT_CLIP_GATHER, 0.0, clip_gather_kernel<true>, grid, dim3(CG_THREADS), 0, (hipStream_t)stream, p);
    return isr_launch(ISR_VARIANT_CLIP_GATHER, 0.0, clip_gather_kernel<false>, grid, dim3(CG_THREADS), 0, (hipStream_t)stream, p);
}

}  // extern "C"
