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
//
// The clips themselves are made on the device too (datagen.py; isrClipPackFrame, isrClipCoverage):
//
//   clip_pack_kernel<VEC>     ONE launch per rendered frame turns the two G-buffers ([h][w][12] and [r h][r w][12], pixel-interleaved)
//                             and the filled flow into the frame's planes inside the flat clip buffers: high <- channels 3..7 and 10, low
//                             <- channels 3..7, channel 3 (alpha) as clamp(a, 0, 1) 2 - 1, everything else copied.  A plane of a frame is
//                             its pixels in G-buffer order, so the work is a transposition of [pixels][12] into [planes][pixels].  A
//                             wave takes 64 consecutive pixels = 3072 contiguous bytes: three 16-byte loads per lane, fully coalesced;
//                             the 48 dwords of a lane go to the wave's LDS tile [12][CP_STRIDE] float by float, and come back as rows.
//     VEC             : a row of four pixels of one plane is one 16-byte LDS read and one 16-byte store (pixel count a multiple of four,
//                       16-byte aligned destinations).
//     otherwise       : a lane stores its pixel of every plane, float by float.
//     CP_STRIDE = 68  : a half-wave's 32 lanes write channel groups 0-3 / 4-7 / 8-11 of eleven consecutive pixels; 4 x 68 = 16 (mod 32)
//                       puts the groups 16 banks apart, so no bank takes more than two of them -- which a 4-byte LDS write absorbs in
//                       its own issue time -- and rows stay 16-byte aligned for the reads (a stride of 64 would be three-way).
//   clip_coverage_kernel      one workgroup per (clip, first / last frame): the summed-area table [H + 1][W + 1] (int32) of the
//                             indicator (c0 + c1) + c2 > 0 of the low-resolution frame, so that the host's crop sampling needs four
//                             table look-ups per candidate instead of the frames.  Row prefixes, a barrier, column prefixes.
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

// ---- the frame packer of the clip generator ----------------------------------------------------------------------------------------
constexpr int CP_THREADS = 256;
constexpr int CP_WAVE_PIXELS = 64;               // one pixel per lane
constexpr int CP_GROUP_PIXELS = CP_THREADS;      // four waves
constexpr int CP_GBUF = 12;                      // floats of a G-buffer pixel
constexpr int CP_STRIDE = 68;                    // floats between the channel rows of a wave's LDS tile (see above)
constexpr int CP_FLOW_FLOATS = 4 * CP_THREADS;   // of the flow copy, per workgroup
constexpr int CP_HIGH_PLANES = 6, CP_LOW_PLANES = 5;
constexpr long long CP_MAX_PIXELS = 1ll << 26;   // of one image: 12 floats per pixel stay below 2^31
constexpr int ISR_VARIANT_CLIP_PACK = 61;        // ops.VARIANT_NAMES
constexpr int ISR_VARIANT_CLIP_COVERAGE = 62;

struct ClipPackParams {
    const float* lowG; const float* highG; const float* flowIn;      // [n][12], [nHigh][12], [2][n]
    float* high; float* low; float* flow;                            // the frame's first plane in each flat buffer
    unsigned n, nHigh, groupsHigh, groupsLow;
};

// alpha -> mask in [-1, 1]: numpy's clip keeps a NaN, and so do the comparisons; the doubling is exact, so x 2 - 1 rounds once, fused or not
__device__ __forceinline__ float pack_mask(float a)
{
    a = a < 0.0f ? 0.0f : (a > 1.0f ? 1.0f : a);
    return a * 2.0f - 1.0f;
}

template <bool VEC>
__global__ void __launch_bounds__(CP_THREADS) clip_pack_kernel(const ClipPackParams p)
{
    __shared__ __attribute__((aligned(16))) float tiles[CP_THREADS / CP_WAVE_PIXELS][CP_GBUF * CP_STRIDE];
    unsigned g = blockIdx.x;
    if (g >= p.groupsHigh + p.groupsLow) {                           // the flow: a copy
        const unsigned total = 2u * p.n, base = (g - p.groupsHigh - p.groupsLow) * CP_FLOW_FLOATS;
        if (VEC) {
            const unsigned e = base + 4u * threadIdx.x;
            if (e < total) *reinterpret_cast<float4*>(p.flow + e) = *reinterpret_cast<const float4*>(p.flowIn + e);
        } else {
            for (unsigned e = base + threadIdx.x; e < total && e < base + CP_FLOW_FLOATS; e += CP_THREADS) p.flow[e] = p.flowIn[e];
        }
        return;
    }
    const bool isHigh = g < p.groupsHigh;
    if (!isHigh) g -= p.groupsHigh;
    const float* src = isHigh ? p.highG : p.lowG;
    float* dst = isHigh ? p.high : p.low;
    const unsigned n = isHigh ? p.nHigh : p.n, planes = isHigh ? CP_HIGH_PLANES : CP_LOW_PLANES;
    const unsigned wave = threadIdx.x / CP_WAVE_PIXELS, lane = threadIdx.x % CP_WAVE_PIXELS;
    const unsigned first = g * CP_GROUP_PIXELS + wave * CP_WAVE_PIXELS;            // the wave's first pixel
    const unsigned valid = first < n ? (n - first < CP_WAVE_PIXELS ? n - first : CP_WAVE_PIXELS) : 0u;
    float* tile = tiles[wave];
    const float4* src4 = reinterpret_cast<const float4*>(src + (size_t)first * CP_GBUF);
    for (unsigned k = 0; k < 3; ++k) {
        const unsigned q = lane + k * CP_WAVE_PIXELS;                 // 16-byte piece q of the wave's 3 x valid: pixel q / 3, channels 4 (q % 3) ...
        if (q < 3u * valid) {
            const float4 a = src4[q];
            const unsigned pix = q / 3u, ch = (q - 3u * pix) * 4u;
            float* t = tile + ch * CP_STRIDE + pix;
            t[0] = a.x; t[CP_STRIDE] = a.y; t[2 * CP_STRIDE] = a.z; t[3 * CP_STRIDE] = a.w;
        }
    }
    __syncthreads();
    if (VEC) {                                                        // n is a multiple of four, and so are first and valid
        const unsigned quads = valid / 4u;
        for (unsigned item = lane; item < planes * 16u; item += CP_WAVE_PIXELS) {
            const unsigned plane = item / 16u, m = item % 16u;
            if (m < quads) {
                const unsigned ch = plane < 5u ? 3u + plane : 10u;
                float4 v = *reinterpret_cast<const float4*>(tile + ch * CP_STRIDE + 4u * m);
                if (plane == 0u) { v.x = pack_mask(v.x); v.y = pack_mask(v.y); v.z = pack_mask(v.z); v.w = pack_mask(v.w); }
                *reinterpret_cast<float4*>(dst + (size_t)plane * n + first + 4u * m) = v;
            }
        }
    } else if (lane < valid) {
        for (unsigned plane = 0; plane < planes; ++plane) {
            const unsigned ch = plane < 5u ? 3u + plane : 10u;
            const float v = tile[ch * CP_STRIDE + lane];
            dst[(size_t)plane * n + first + lane] = plane == 0u ? pack_mask(v) : v;
        }
    }
}

// pixels of the low image and of the high one, or -1 where the shape is not one the kernel takes
long long cp_pixels(int h, int w, int r, long long* high)
{
    if (h <= 0 || w <= 0 || r <= 0 || r > 64) return -1;
    const long long n = (long long)h * w, nh = n * r * r;
    if (nh > CP_MAX_PIXELS) return -1;
    if (high) *high = nh;
    return n;
}

// ---- crop coverage of the first and last frame of every clip ------------------------------------------------------------------------
constexpr int CC_THREADS = 256;

__global__ void __launch_bounds__(CC_THREADS) clip_coverage_kernel(const float* __restrict__ low, const long long* __restrict__ clips,
                                                                   const long long* __restrict__ tableOffsets, int* __restrict__ tables,
                                                                   int T, int Cl)
{
    const long long* clip = clips + (long long)(blockIdx.x >> 1) * CG_CLIP_WORDS;
    const unsigned H = (unsigned)clip[3], W = (unsigned)clip[4];
    const size_t plane = (size_t)H * W;
    const float* frame = low + clip[1] + ((blockIdx.x & 1) ? (size_t)(T - 1) * Cl * plane : 0);
    const unsigned Ws = W + 1u;
    int* sat = tables + tableOffsets[blockIdx.x >> 1] + ((blockIdx.x & 1) ? (size_t)(H + 1u) * Ws : 0);
    for (unsigned x = threadIdx.x; x < Ws; x += CC_THREADS) sat[x] = 0;
    for (unsigned y = threadIdx.x; y < H; y += CC_THREADS) {          // row prefixes
        const float* c0 = frame + (size_t)y * W;
        int* row = sat + (size_t)(y + 1u) * Ws;
        int sum = 0;
        row[0] = 0;
        for (unsigned x = 0; x < W; ++x) {
            sum += ((c0[x] + c0[plane + x]) + c0[2 * plane + x]) > 0.0f ? 1 : 0;
            row[x + 1u] = sum;
        }
    }
    __syncthreads();
    for (unsigned x = threadIdx.x + 1u; x < Ws; x += CC_THREADS) {    // column prefixes
        int sum = 0;
        for (unsigned y = 1; y <= H; ++y) {
            sum += sat[(size_t)y * Ws + x];
            sat[(size_t)y * Ws + x] = sum;
        }
    }
}

}  // namespace

extern "C" {

int isrClipPackFrameSupported(int h, int w, int r) { return cp_pixels(h, w, r, nullptr) > 0 ? 1 : 0; }

int isrClipPackFrame(const float* lowGbuffer, const float* highGbuffer, const float* flow, int h, int w, int r, float* highBuf,
                     long long highOffset, float* lowBuf, long long lowOffset, float* flowBuf, long long flowOffset, void* stream)
{
    if (!lowGbuffer || !highGbuffer || !flow || !highBuf || !lowBuf || !flowBuf || highOffset < 0 || lowOffset < 0 || flowOffset < 0) return -1;
    long long nh = 0;
    const long long n = cp_pixels(h, w, r, &nh);
    if (n <= 0 || !aligned16(lowGbuffer) || !aligned16(highGbuffer)) return -3;     // the loads are 16 bytes wide in both forms
    ClipPackParams p;
    p.lowG = lowGbuffer; p.highG = highGbuffer; p.flowIn = flow;
    p.high = highBuf + highOffset; p.low = lowBuf + lowOffset; p.flow = flowBuf + flowOffset;
    p.n = (unsigned)n; p.nHigh = (unsigned)nh;
    p.groupsHigh = (unsigned)((nh + CP_GROUP_PIXELS - 1) / CP_GROUP_PIXELS);
    p.groupsLow = (unsigned)((n + CP_GROUP_PIXELS - 1) / CP_GROUP_PIXELS);
    const unsigned groupsFlow = (unsigned)((2 * n + CP_FLOW_FLOATS - 1) / CP_FLOW_FLOATS);
    const bool vec = (w & 3) == 0 && aligned16(flow) && aligned16(p.high) && aligned16(p.low) && aligned16(p.flow);
    const dim3 grid(p.groupsHigh + p.groupsLow + groupsFlow);
    if (vec) return isr_launch(ISR_VARIANT_CLIP_PACK, 0.0, clip_pack_kernel<true>, grid, dim3(CP_THREADS), 0, (hipStream_t)stream, p);
    return isr_launch(ISR_VARIANT_CLIP_PACK, 0.0, clip_pack_kernel<false>, grid, dim3(CP_THREADS), 0, (hipStream_t)stream, p);
}

int isrClipCoverageSupported(int numClips, int T, int Cl) { return numClips > 0 && numClips <= (1 << 30) && T > 0 && Cl >= 3 ? 1 : 0; }

int isrClipCoverage(const float* low, const long long* clipTable, const long long* tableOffsets, int numClips, int T, int Cl, int* tables,
                    void* stream)
{
    if (!low || !clipTable || !tableOffsets || !tables) return -1;
    if (!isrClipCoverageSupported(numClips, T, Cl)) return -3;
    return isr_launch(ISR_VARIANT_CLIP_COVERAGE, 0.0, clip_coverage_kernel, dim3(2u * (unsigned)numClips), dim3(CC_THREADS), 0,
                      (hipStream_t)stream, low, clipTable, tableOffsets, tables, T, Cl);
}

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
