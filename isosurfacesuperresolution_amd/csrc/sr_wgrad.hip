// Weight gradient of the 3x3 convolution (gfx950): the exact fp32 kernels, the bf16 and the split-operand kernels, the scale and
// reduction kernels they share, and ONE host path for all of them -- wgrad_fill / wgrad_plan / wgrad_launch, the shape DESIGN.md 4.5
// describes for the forward dispatchers.  The isrConv*WeightGrad* entry points at the end are thin calls of these three.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sr_conv_common.h"
#include "sr_split_scale.h"

namespace {

// ---- weight gradient -------------------------------------------------------------------------
// dW[co][ci][tap] = sum_pixels gz[co][p] * x[ci][p + tap]:  M = co (A = gz), N = ci (B = x patch),
// K = pixels.  A workgroup walks pixel tiles of 4 rows x 32 cols (grid-stride), keeps its 64x64x9
// partial sums in registers (wave (m,n) owns the 32x32 block (m,n) for all 9 taps = 144 VGPRs) and
// writes one slab; a second kernel reduces the slabs in a fixed order (bitwise reproducible, no
// float atomics).  LDS planes are padded to odd strides: lanes 0-31 index the channel.
constexpr int WG_TH = 4, WG_TW = 32;
constexpr int WG_PX = WG_TH * WG_TW;          // 128 pixels per tile
constexpr int GZ_STRIDE = WG_PX + 1;          // 129
constexpr int XP_W = WG_TW + 2;               // 34
constexpr int XP_PLANE = (WG_TH + 2) * XP_W + 1;   // 205

constexpr int WG_MAX_SEG = 32;
struct WGradParams {
    // K runs over the pixels of `segments` tensor pairs of N images each (the frames of a training clip share the
    // weights, so one launch can take all of them: train.py defers the weight gradients to the end of the backward)
    const float* x[WG_MAX_SEG];     // each [N][Cin][H][W]
    const float* gz[WG_MAX_SEG];    // each [N][Cout][H][W]
    float* slabs;       // [G][9][64][64]
    float* bslabs;      // [G][64] partial sums of gz per output channel (bias gradient), or NULL
    int N, Cin, H, W, Cout;
    int ci0, co0;       // channel group handled by this launch
    int tilesX, tilesY, ntiles;
    const float* scale; // split-operand kernel only: { 2^S, 2^-S } with max |gz| 2^S in [2^13, 2^14)
    ISR_DIAG_MEMBER(int, dbg, 0);            // diagnostics (isrDebugSetAblation; conv3x3_wgrad_split2_kernel): 1 no MFMAs, 2 no split / park, 4 no fetch
};

// Staging is branch-free and software pipelined: the next tile's 8 + 51 elements per thread are fetched through
// buffer descriptors (out-of-image / out-of-range channels read 0) into registers BEFORE the tile's MFMA block and
// parked in LDS after it.  TAPS = 9: one workgroup accumulates all taps (144 accumulator registers per wave);
// TAPS = 3: three workgroups share a tile set, one row of the 3x3 each -- three times the workgroups for small
// problems (the 32x32 training crops are 128 tiles for 256 CUs).
// KSPLIT (at most 32 output channels in this launch, e.g. the 64 -> 6 output layer): instead of idling on an empty
// second channel block, the waves m = 1 take rows 2..3 of every tile and the waves m = 0 rows 0..1, each pair writes
// its own slab (g and G + g) -- half the MFMAs per workgroup.
template <int TAPS, bool KSPLIT = false>
__global__ __launch_bounds__(NTHREADS, 1) void conv3x3_wgrad_kernel(const WGradParams p)
{
    __shared__ float gzs[64 * GZ_STRIDE];
    __shared__ float xps[64 * XP_PLANE];
    constexpr int TG = 9 / TAPS;                       // workgroups per slab
    constexpr int NGZ = 64 * WG_PX / NTHREADS;         // 32 gz elements per thread and tile
    constexpr int NXE = (64 * (WG_TH + 2) * XP_W + NTHREADS - 1) / NTHREADS;   // 51 x elements
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = wave >> 1, nn = wave & 1;
    const int j = lane & 31, kh = lane >> 5;
    const int g = blockIdx.x / TG, tap0 = (blockIdx.x - g * TG) * TAPS, nslab = gridDim.x / TG;

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

    // per-thread element descriptors, tile invariant: gz element i = (channel c, pixel px) -> LDS slot + (ry, rx);
    // x element i = (channel c, patch row r, patch column col)
    unsigned xdesc[NXE];
#pragma unroll
    for (int i = 0; i < NXE; ++i) {
        const int e = tid + i * NTHREADS;
        const int c = e / ((WG_TH + 2) * XP_W), rem = e - c * ((WG_TH + 2) * XP_W);
        const int r = rem / XP_W, col = rem - r * XP_W;
        xdesc[i] = e < 64 * (WG_TH + 2) * XP_W ? (unsigned)(c | (r << 8) | (col << 16)) : 0xFFFFFFFFu;
    }
    const size_t planeBytes = (size_t)p.H * p.W * 4;
    const int tilesPerImage = p.tilesX * p.tilesY;
    float gv[NGZ], xv[NXE];

    auto fetch = [&](int tile) {
        const int ng = tile / tilesPerImage;             // image index over all segments
        const int t2 = tile - ng * tilesPerImage;
        const int seg = ng / p.N, n = ng - seg * p.N;
        const int ty = t2 / p.tilesX, tx = t2 - ty * p.tilesX;
        const int oy0 = ty * WG_TH, ox0 = tx * WG_TW;
        const int gzc = p.Cout - p.co0, xc = p.Cin - p.ci0;
        const rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gz[seg] + ((size_t)n * p.Cout + p.co0) * p.H * p.W), 0,
                                                             (int)((gzc < 64 ? gzc : 64) * planeBytes), 0x00020000);
        const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x[seg] + ((size_t)n * p.Cin + p.ci0) * p.H * p.W), 0,
                                                             (int)((xc < 64 ? xc : 64) * planeBytes), 0x00020000);
#pragma unroll
        for (int i = 0; i < NGZ; ++i) {
            const int e = tid + i * NTHREADS;
            const int c = e >> 7, px = e & 127, ry = px >> 5, rx = px & 31;
            const int gy = oy0 + ry, gx = ox0 + rx;
            const bool ok = gy < p.H && gx < p.W;
            gv[i] = buf_load(grs, ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BAD_OFFSET);
        }
#pragma unroll
        for (int i = 0; i < NXE; ++i) {
            const unsigned d = xdesc[i];
            const int c = d & 255, r = (d >> 8) & 255, col = (d >> 16) & 255;
            const int gy = oy0 + r - 1, gx = ox0 + col - 1;
            const bool ok = d != 0xFFFFFFFFu && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            xv[i] = buf_load(xrs, ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BAD_OFFSET);
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < NGZ; ++i) {
            const int e = tid + i * NTHREADS;
            gzs[(e >> 7) * GZ_STRIDE + (e & 127)] = gv[i];
        }
#pragma unroll
        for (int i = 0; i < NXE; ++i) {
            const unsigned d = xdesc[i];
            if (d != 0xFFFFFFFFu) xps[(d & 255) * XP_PLANE + ((d >> 8) & 255) * XP_W + ((d >> 16) & 255)] = xv[i];
        }
    };

    float bsum = 0.0f;                                   // this lane's share of sum(gz[co = m*32+j]) (pixels kh, kh+2, ..)
    int tile = g;
    if (tile < p.ntiles) { fetch(tile); park(); }
    __syncthreads();
    for (; tile < p.ntiles; tile += nslab) {
        const bool more = tile + nslab < p.ntiles;
        if (more) fetch(tile + nslab);
        __builtin_amdgcn_sched_barrier(0);               // the loads stay above the MFMA block
        const float* ga = &gzs[((KSPLIT ? 0 : m * 32) + j) * GZ_STRIDE + kh];
        const float* xb = &xps[(nn * 32 + j) * XP_PLANE + kh];
#pragma unroll
        for (int r2 = 0; r2 < (KSPLIT ? WG_TH / 2 : WG_TH); ++r2) {
            const int ry = KSPLIT ? m * (WG_TH / 2) + r2 : r2;
#pragma unroll 4
            for (int rx = 0; rx < WG_TW; rx += 2) {
                const float a = ga[ry * WG_TW + rx];
                bsum += a;
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    const int tap = TAPS == 9 ? t : -1;
                    const int dy = TAPS == 9 ? tap / 3 : 0, dx = TAPS == 9 ? tap - dy * 3 : t;
                    const float b = xb[(ry + (TAPS == 9 ? dy : tap0 / 3)) * XP_W + rx + dx];
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                 // everyone has finished reading this tile
        if (more) park();
        __syncthreads();
    }
    // slab[g][tap][co(64)][ci(64)]
    const int gs = KSPLIT ? g + m * nslab : g;        // KSPLIT: slabs [0, G) hold rows 0..1, [G, 2G) rows 2..3; channels 32.. stay 0
    float* slab = p.slabs + (size_t)gs * 9 * 64 * 64;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = (KSPLIT ? 0 : m * 32) + (i & 3) + 8 * (i >> 2) + 4 * kh;
            slab[((size_t)(tap0 + t) * 64 + co) * 64 + nn * 32 + j] = acc[t][i];
        }
    // bias gradient: the A operand already passes every gz value of the tile set through the waves with nn == 0
    const float btot = bsum + __shfl_xor(bsum, 32, 64);
    if (p.bslabs && nn == 0 && tap0 == 0 && kh == 0) p.bslabs[(size_t)gs * 64 + (KSPLIT ? 0 : m * 32) + j] = btot;
}

// ---- weight gradient with bf16 operands (the opt-in mixed-precision training mode, not the parity step) ----------------
// Same decomposition (M = co, N = ci, K = pixels of 4x32 tiles, one slab per workgroup, the same reduction), but the
// tile is rounded to bf16 on its way into LDS and multiplied by v_mfma_f32_32x32x16_bf16 (16 pixels per instruction):
// A fragment = 8 consecutive pixels of one gz channel (one ds_read_b128 from [co][pixel]), B fragment = 8 consecutive
// pixels of one x channel SHIFTED by the tap: the row is read once as five dwords (10 pixels) and the three horizontal
// taps are dwords 0..3, the 16-bit funnel shifts of neighbouring dwords, and dwords 1..4 -- no shifted copies in LDS.
// At this MFMA rate the kernel is bound by streaming the tile (84 KB per 2300 MFMA cycles).  Needs W % 4 == 0.
typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
constexpr int BG_PITCH = 272;                  // bytes per gz channel row in LDS: 128 pixels x 2 + 16 (bank spread)
constexpr int BX_ROW = 80;                     // bytes per x patch row: 40 pixels (34 used), 16-byte aligned rows
constexpr int BX_PITCH = 6 * BX_ROW + 16;      // 496 bytes per x channel
constexpr int BX_PAIRS = 17;                   // packed pixel pairs per patch row (34 columns)

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi)
{
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    bf2 v; v[0] = (__bf16)lo; v[1] = (__bf16)hi;
    return __builtin_bit_cast(unsigned, v);
}

__global__ __launch_bounds__(NTHREADS, 1) void conv3x3_wgrad_bf16_kernel(const WGradParams p)
{
    __shared__ __attribute__((aligned(16))) unsigned char gzs[64 * BG_PITCH];
    __shared__ __attribute__((aligned(16))) unsigned char xps[64 * BX_PITCH];
    constexpr int NGQ = 64 * WG_PX / 4 / NTHREADS;                              // 8 gz quads per thread and tile
    constexpr int NXP = (64 * (WG_TH + 2) * BX_PAIRS + NTHREADS - 1) / NTHREADS;  // 26 x pairs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = wave >> 1, nn = wave & 1;
    const int j = lane & 31, kh = lane >> 5;
    const int g = blockIdx.x, nslab = gridDim.x;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    float bs[NGQ];                                                             // fp32 sums of gz per thread (channel tid/32 + 8 i)
#pragma unroll
    for (int i = 0; i < NGQ; ++i) bs[i] = 0.0f;

    const size_t planeBytes = (size_t)p.H * p.W * 4;
    const int tilesPerImage = p.tilesX * p.tilesY;
    u32x4 gq[NGQ];
    float xlo[NXP], xhi[NXP];

    auto fetch = [&](int tile) {
        const int ng = tile / tilesPerImage;
        const int t2 = tile - ng * tilesPerImage;
        const int seg = ng / p.N, n = ng - seg * p.N;
        const int ty = t2 / p.tilesX, tx = t2 - ty * p.tilesX;
        const int oy0 = ty * WG_TH, ox0 = tx * WG_TW;
        const int gzc = p.Cout - p.co0, xc = p.Cin - p.ci0;
        const rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gz[seg] + ((size_t)n * p.Cout + p.co0) * p.H * p.W), 0,
                                                             (int)((gzc < 64 ? gzc : 64) * planeBytes), 0x00020000);
        const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x[seg] + ((size_t)n * p.Cin + p.ci0) * p.H * p.W), 0,
                                                             (int)((xc < 64 ? xc : 64) * planeBytes), 0x00020000);
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {                                        // quad q = (channel q / 32, 4 pixels)
            const int q = tid + i * NTHREADS;
            const int c = q >> 5, px = (q & 31) * 4, ry = px >> 5, rx = px & 31;
            const int gy = oy0 + ry, gx = ox0 + rx;
            const bool ok = gy < p.H && gx < p.W;                              // W % 4 == 0: a quad is inside or outside as a whole
            gq[i] = __builtin_amdgcn_raw_buffer_load_b128(grs, (int)(ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BAD_OFFSET), 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NXP; ++i) {                                        // pair e = (channel, patch row, patch columns 2 pr, 2 pr + 1)
            const int e = tid + i * NTHREADS;
            const int c = e / ((WG_TH + 2) * BX_PAIRS), rem = e - c * ((WG_TH + 2) * BX_PAIRS);
            const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
            const int gy = oy0 + r - 1, gx = ox0 + 2 * pr - 1;
            const bool in = e < 64 * (WG_TH + 2) * BX_PAIRS && (unsigned)gy < (unsigned)p.H;
            const unsigned off = (unsigned)((c * p.H + gy) * p.W + gx) * 4u;
            xlo[i] = buf_load(xrs, (in && (unsigned)gx < (unsigned)p.W) ? off : BAD_OFFSET);
            xhi[i] = buf_load(xrs, (in && (unsigned)(gx + 1) < (unsigned)p.W) ? off + 4u : BAD_OFFSET);
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {
            const int q = tid + i * NTHREADS;
            const float4 f = __builtin_bit_cast(float4, gq[i]);
            bs[i] += (f.x + f.y) + (f.z + f.w);
            uint2 v; v.x = pack_bf16(f.x, f.y); v.y = pack_bf16(f.z, f.w);
            *reinterpret_cast<uint2*>(gzs + (q >> 5) * BG_PITCH + (q & 31) * 8) = v;
        }
#pragma unroll
        for (int i = 0; i < NXP; ++i) {
            const int e = tid + i * NTHREADS;
            if (e < 64 * (WG_TH + 2) * BX_PAIRS) {
                const int c = e / ((WG_TH + 2) * BX_PAIRS), rem = e - c * ((WG_TH + 2) * BX_PAIRS);
                const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
                *reinterpret_cast<unsigned*>(xps + c * BX_PITCH + r * BX_ROW + pr * 4) = pack_bf16(xlo[i], xhi[i]);
            }
        }
    };

    int tile = g;
    if (tile < p.ntiles) { fetch(tile); park(); }
    __syncthreads();
    for (; tile < p.ntiles; tile += nslab) {
        const bool more = tile + nslab < p.ntiles;
        if (more) fetch(tile + nslab);
        __builtin_amdgcn_sched_barrier(0);
        const unsigned char* ga = gzs + (m * 32 + j) * BG_PITCH + kh * 16;
        const unsigned char* xb = xps + (nn * 32 + j) * BX_PITCH + kh * 16;
#pragma unroll
        for (int ry = 0; ry < WG_TH; ++ry) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {                                   // k-step = 16 pixels of the row: columns 16 ks + 8 kh ..
                const wbf16x8 a = __builtin_bit_cast(wbf16x8, *reinterpret_cast<const u32x4*>(ga + (ry * 32 + ks * 16) * 2));
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const unsigned char* row = xb + (ry + dy) * BX_ROW + ks * 32;
                    const u32x4 d = *reinterpret_cast<const u32x4*>(row);
                    const unsigned d4 = *reinterpret_cast<const unsigned*>(row + 16);
                    u32x4 f1, f2;
                    f1.x = __builtin_amdgcn_alignbit(d.y, d.x, 16); f1.y = __builtin_amdgcn_alignbit(d.z, d.y, 16);
                    f1.z = __builtin_amdgcn_alignbit(d.w, d.z, 16); f1.w = __builtin_amdgcn_alignbit(d4, d.w, 16);
                    f2.x = d.y; f2.y = d.z; f2.z = d.w; f2.w = d4;
                    acc[dy * 3 + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(wbf16x8, d), acc[dy * 3 + 0], 0, 0, 0);
                    acc[dy * 3 + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(wbf16x8, f1), acc[dy * 3 + 1], 0, 0, 0);
                    acc[dy * 3 + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(wbf16x8, f2), acc[dy * 3 + 2], 0, 0, 0);
                }
            }
        }
        __syncthreads();
        if (more) park();
        __syncthreads();
    }
    float* slab = p.slabs + (size_t)g * 9 * 64 * 64;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = m * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
            slab[((size_t)t * 64 + co) * 64 + nn * 32 + j] = acc[t][i];
        }
    // bias gradient from the fp32 values: thread t's sum i belongs to channel t / 32 + 8 i; reduce over the 32 lanes
    if (p.bslabs) {
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {
            float v = bs[i];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((lane & 31) == 0) p.bslabs[(size_t)g * 64 + (tid >> 5) + 8 * i] = v;
        }
    }
}

// ---- weight gradient on split operands: fp32-equivalent accuracy on the fp16 matrix pipe (the training default) --------
// The decomposition and tile pipeline of conv3x3_wgrad_bf16_kernel, with every operand carried as two fp16 numbers
// (csrc/sr_conv_split.hip): gz, whose magnitude is unknown, is first scaled by a power of two taken from max |gz| over
// the launch's tensors (wgrad_absmax / wgrad_scale kernels; undone exactly by the slab reduction) and split as
// hi = RN16(g), lo = RN16(g - hi); x is split as hi = RN16(x), lo' = RN16((x - hi) 2^11) and meets gz_hi 2^-11 (an
// exponent shift of the A fragment in registers).  A product is gz_lo x_hi + (gz_hi 2^-11) x_lo' + gz_hi x_hi: three
// v_mfma_f32_32x32x16_f16 instead of eight v_mfma_f32_32x32x2_f32 at twice the cycles each -> 5.3x fewer matrix cycles.
typedef _Float16 wf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_pair(float a, float b, float lo_scale, unsigned& hi, unsigned& lo)
{
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 vh, vl;
    vh[0] = (_Float16)a; vh[1] = (_Float16)b;
    vl[0] = (_Float16)((a - (float)vh[0]) * lo_scale); vl[1] = (_Float16)((b - (float)vh[1]) * lo_scale);
    hi = __builtin_bit_cast(unsigned, vh); lo = __builtin_bit_cast(unsigned, vl);
}

// form 1 (one wave per SIMD): diagnostics builds only -- isrDebugSetWgradSplitForm, the form-parity test
#ifdef ISR_DIAG
constexpr int WS_LDS_BYTES = 2 * (64 * BG_PITCH + 64 * BX_PITCH);          // hi and lo planes of gz and x: 98 304 B

__global__ __launch_bounds__(NTHREADS, 1) void conv3x3_wgrad_split_kernel(const WGradParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char wsl[];
    unsigned char* gzh = wsl;
    unsigned char* gzl = gzh + 64 * BG_PITCH;
    unsigned char* xph = gzl + 64 * BG_PITCH;
    unsigned char* xpl = xph + 64 * BX_PITCH;
    constexpr int NGQ = 64 * WG_PX / 4 / NTHREADS;                              // 8 gz quads per thread and tile
    constexpr int NXP = (64 * (WG_TH + 2) * BX_PAIRS + NTHREADS - 1) / NTHREADS;  // 26 x pairs
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = wave >> 1, nn = wave & 1;
    const int j = lane & 31, kh = lane >> 5;
    const int g = blockIdx.x, nslab = gridDim.x;
    const float gscale = p.scale[0];

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
    float bs[NGQ];                                                             // fp32 sums of gz per thread (channel tid/32 + 8 i)
#pragma unroll
    for (int i = 0; i < NGQ; ++i) bs[i] = 0.0f;

    const size_t planeBytes = (size_t)p.H * p.W * 4;
    const int tilesPerImage = p.tilesX * p.tilesY;
    u32x4 gq[NGQ];
    float xlo[NXP], xhi[NXP];

    auto fetch = [&](int tile) {
        const int ng = tile / tilesPerImage;
        const int t2 = tile - ng * tilesPerImage;
        const int seg = ng / p.N, n = ng - seg * p.N;
        const int ty = t2 / p.tilesX, tx = t2 - ty * p.tilesX;
        const int oy0 = ty * WG_TH, ox0 = tx * WG_TW;
        const int gzc = p.Cout - p.co0, xc = p.Cin - p.ci0;
        const rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gz[seg] + ((size_t)n * p.Cout + p.co0) * p.H * p.W), 0,
                                                             (int)((gzc < 64 ? gzc : 64) * planeBytes), 0x00020000);
        const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x[seg] + ((size_t)n * p.Cin + p.ci0) * p.H * p.W), 0,
                                                             (int)((xc < 64 ? xc : 64) * planeBytes), 0x00020000);
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {                                        // quad q = (channel q / 32, 4 pixels)
            const int q = tid + i * NTHREADS;
            const int c = q >> 5, px = (q & 31) * 4, ry = px >> 5, rx = px & 31;
            const int gy = oy0 + ry, gx = ox0 + rx;
            const bool ok = gy < p.H && gx < p.W;                              // W % 4 == 0: a quad is inside or outside as a whole
            gq[i] = __builtin_amdgcn_raw_buffer_load_b128(grs, (int)(ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BAD_OFFSET), 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NXP; ++i) {                                        // pair e = (channel, patch row, patch columns 2 pr, 2 pr + 1)
            const int e = tid + i * NTHREADS;
            const int c = e / ((WG_TH + 2) * BX_PAIRS), rem = e - c * ((WG_TH + 2) * BX_PAIRS);
            const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
            const int gy = oy0 + r - 1, gx = ox0 + 2 * pr - 1;
            const bool in = e < 64 * (WG_TH + 2) * BX_PAIRS && (unsigned)gy < (unsigned)p.H;
            const unsigned off = (unsigned)((c * p.H + gy) * p.W + gx) * 4u;
            xlo[i] = buf_load(xrs, (in && (unsigned)gx < (unsigned)p.W) ? off : BAD_OFFSET);
            xhi[i] = buf_load(xrs, (in && (unsigned)(gx + 1) < (unsigned)p.W) ? off + 4u : BAD_OFFSET);
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {
            const int q = tid + i * NTHREADS;
            const float4 f = __builtin_bit_cast(float4, gq[i]);
            bs[i] += (f.x + f.y) + (f.z + f.w);
            uint2 vh, vl;
            split_pair(f.x * gscale, f.y * gscale, 1.0f, vh.x, vl.x);
            split_pair(f.z * gscale, f.w * gscale, 1.0f, vh.y, vl.y);
            *reinterpret_cast<uint2*>(gzh + (q >> 5) * BG_PITCH + (q & 31) * 8) = vh;
            *reinterpret_cast<uint2*>(gzl + (q >> 5) * BG_PITCH + (q & 31) * 8) = vl;
        }
#pragma unroll
        for (int i = 0; i < NXP; ++i) {
            const int e = tid + i * NTHREADS;
            if (e < 64 * (WG_TH + 2) * BX_PAIRS) {
                const int c = e / ((WG_TH + 2) * BX_PAIRS), rem = e - c * ((WG_TH + 2) * BX_PAIRS);
                const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
                unsigned vh, vl;
                split_pair(xlo[i], xhi[i], 2048.0f, vh, vl);
                *reinterpret_cast<unsigned*>(xph + c * BX_PITCH + r * BX_ROW + pr * 4) = vh;
                *reinterpret_cast<unsigned*>(xpl + c * BX_PITCH + r * BX_ROW + pr * 4) = vl;
            }
        }
    };

    int tile = g;
    if (tile < p.ntiles) { fetch(tile); park(); }
    __syncthreads();
    for (; tile < p.ntiles; tile += nslab) {
        const bool more = tile + nslab < p.ntiles;
        if (more) fetch(tile + nslab);
        __builtin_amdgcn_sched_barrier(0);
        const int ga = (m * 32 + j) * BG_PITCH + kh * 16;
        const int xb = (nn * 32 + j) * BX_PITCH + kh * 16;
#pragma unroll
        for (int ry = 0; ry < WG_TH; ++ry) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {                                   // k-step = 16 pixels of the row: columns 16 ks + 8 kh ..
                const wf16x8 ah = __builtin_bit_cast(wf16x8, *reinterpret_cast<const u32x4*>(gzh + ga + (ry * 32 + ks * 16) * 2));
                const wf16x8 al = __builtin_bit_cast(wf16x8, *reinterpret_cast<const u32x4*>(gzl + ga + (ry * 32 + ks * 16) * 2));
                const wf16x8 as = ah * (_Float16)0.00048828125f;              // gz_hi 2^-11: partner of the scaled x_lo'
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int row = xb + (ry + dy) * BX_ROW + ks * 32;
                    const u32x4 dh = *reinterpret_cast<const u32x4*>(xph + row);
                    const unsigned dh4 = *reinterpret_cast<const unsigned*>(xph + row + 16);
                    const u32x4 dl = *reinterpret_cast<const u32x4*>(xpl + row);
                    const unsigned dl4 = *reinterpret_cast<const unsigned*>(xpl + row + 16);
                    u32x4 h1, h2, l1, l2;
                    h1.x = __builtin_amdgcn_alignbit(dh.y, dh.x, 16); h1.y = __builtin_amdgcn_alignbit(dh.z, dh.y, 16);
                    h1.z = __builtin_amdgcn_alignbit(dh.w, dh.z, 16); h1.w = __builtin_amdgcn_alignbit(dh4, dh.w, 16);
                    h2.x = dh.y; h2.y = dh.z; h2.z = dh.w; h2.w = dh4;
                    l1.x = __builtin_amdgcn_alignbit(dl.y, dl.x, 16); l1.y = __builtin_amdgcn_alignbit(dl.z, dl.y, 16);
                    l1.z = __builtin_amdgcn_alignbit(dl.w, dl.z, 16); l1.w = __builtin_amdgcn_alignbit(dl4, dl.w, 16);
                    l2.x = dl.y; l2.y = dl.z; l2.z = dl.w; l2.w = dl4;
#define ISR_WS3(T, BH, BL)                                                                                              \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, __builtin_bit_cast(wf16x8, BH), acc[T], 0, 0, 0);   \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as, __builtin_bit_cast(wf16x8, BL), acc[T], 0, 0, 0);   \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(wf16x8, BH), acc[T], 0, 0, 0);
                    ISR_WS3(dy * 3 + 0, dh, dl)
                    ISR_WS3(dy * 3 + 1, h1, l1)
                    ISR_WS3(dy * 3 + 2, h2, l2)
#undef ISR_WS3
                }
            }
        }
        __syncthreads();
        if (more) park();
        __syncthreads();
    }
    float* slab = p.slabs + (size_t)g * 9 * 64 * 64;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = m * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
            slab[((size_t)t * 64 + co) * 64 + nn * 32 + j] = acc[t][i];
        }
    // bias gradient from the fp32 values: thread t's sum i belongs to channel t / 32 + 8 i; reduce over the 32 lanes
    if (p.bslabs) {
#pragma unroll
        for (int i = 0; i < NGQ; ++i) {
            float v = bs[i];
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((lane & 31) == 0) p.bslabs[(size_t)g * 64 + (tid >> 5) + 8 * i] = v;
        }
    }
}

#endif  // ISR_DIAG

// ---- the same sums with the staging on its own waves ----------------------------------------------------------------------
// conv3x3_wgrad_split_kernel runs ONE wave per SIMD (144 accumulator registers + 92 of staging: 507 registers), so the split of the
// next tile (a few hundred VALU instructions per thread), its LDS writes and the latency of every operand read sit in series with
// the MFMAs: 8.7 us per 128-pixel tile for 3.4 us of matrix work.  Here a workgroup is EIGHT waves, two per SIMD: waves 0..3 own the
// accumulators and do nothing but read operands and issue MFMAs, waves 4..7 fetch, split and park -- the matrix pipe and the vector
// pipe of a SIMD work for different waves at the same time.  Both roles fit 256 registers (accumulators + operands | two register
// sets of staging).  LDS is double buffered, which a 4-row tile does not fit twice: the unit of the pipeline is HALF a tile (2 rows
// x 32 pixels, 61 KB per buffer); a workgroup walks the tiles of conv3x3_wgrad_split_kernel in the same order, each as its two
// halves, so every accumulator sees the same products in the same order -- slabs and weight gradients are bit-identical.  (The bias
// sums are grouped differently per thread: equal to rounding.)  One barrier per half-tile.
constexpr int W2_THREADS = 512;
constexpr int W2_TH = 2;
constexpr int W2_GP = W2_TH * WG_TW * 2 + 16;                 // bytes per gz channel: 64 pixels x 2 + 16 (bank spread: 36 dwords)
constexpr int W2_XP = (W2_TH + 2) * BX_ROW + 16;              // bytes per x channel: 4 patch rows + 16 (84 dwords)
constexpr int W2_GZ = 64 * W2_GP, W2_X = 64 * W2_XP;
constexpr int W2_BUF = 2 * W2_GZ + 2 * W2_X;                  // hi and lo planes of gz and x: 61 440 B
constexpr int W2_LDS_BYTES = 2 * W2_BUF;                      // 122 880 B
constexpr int W2_NGQ = 64 * W2_TH * WG_TW / 4 / 256;          // 4 gz quads per staging thread and half-tile
constexpr int W2_NXP = 64 * (W2_TH + 2) * BX_PAIRS / 256;     // 17 x pairs (4352 = 17 x 256 exactly)
static_assert(64 * (W2_TH + 2) * BX_PAIRS == W2_NXP * 256, "x pairs divide evenly over the staging threads");

struct W2Stage { u32x4 gq[W2_NGQ]; float xlo[W2_NXP], xhi[W2_NXP]; };

__global__ __launch_bounds__(W2_THREADS, 1) void conv3x3_wgrad_split2_kernel(const WGradParams p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char w2l[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool consumer = wave < 4;
    const int m = (wave >> 1) & 1, nn = wave & 1;
    const int j = lane & 31, kh = lane >> 5;
    const int pt = tid & 255;                                                  // staging thread
    const int g = blockIdx.x, nslab = gridDim.x;
    const int nhalf = g < p.ntiles ? 2 * ((p.ntiles - g + nslab - 1) / nslab) : 0;
    const float gscale = p.scale[0];

    const size_t planeBytes = (size_t)p.H * p.W * 4;
    const int tilesPerImage = p.tilesX * p.tilesY;

    auto fetch = [&](W2Stage& st, int it) {
        const int tile = g + (it >> 1) * nslab;
        const int ng = tile / tilesPerImage;
        const int t2 = tile - ng * tilesPerImage;
        const int seg = ng / p.N, n = ng - seg * p.N;
        const int ty = t2 / p.tilesX, tx = t2 - ty * p.tilesX;
        const int oy0 = ty * WG_TH + (it & 1) * W2_TH, ox0 = tx * WG_TW;
        const int gzc = p.Cout - p.co0, xc = p.Cin - p.ci0;
        const rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.gz[seg] + ((size_t)n * p.Cout + p.co0) * p.H * p.W), 0,
                                                             (int)((gzc < 64 ? gzc : 64) * planeBytes), 0x00020000);
        const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x[seg] + ((size_t)n * p.Cin + p.ci0) * p.H * p.W), 0,
                                                             (int)((xc < 64 ? xc : 64) * planeBytes), 0x00020000);
#pragma unroll
        for (int i = 0; i < W2_NGQ; ++i) {                                     // quad q = (channel q / 16, row, 4 pixels)
            const int q = pt + i * 256;
            const int c = q >> 4, ry = (q >> 3) & 1, rx = (q & 7) * 4;
            const int gy = oy0 + ry, gx = ox0 + rx;
            const bool ok = gy < p.H && gx < p.W;                              // W % 4 == 0: a quad is inside or outside as a whole
            st.gq[i] = __builtin_amdgcn_raw_buffer_load_b128(grs, (int)(ok ? (unsigned)((c * p.H + gy) * p.W + gx) * 4u : BAD_OFFSET), 0, 0);
        }
#pragma unroll
        for (int i = 0; i < W2_NXP; ++i) {                                     // pair e = (channel, patch row, patch columns 2 pr, 2 pr + 1)
            const int e = pt + i * 256;
            const int c = e / ((W2_TH + 2) * BX_PAIRS), rem = e - c * ((W2_TH + 2) * BX_PAIRS);
            const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
            const int gy = oy0 + r - 1, gx = ox0 + 2 * pr - 1;
            const bool in = (unsigned)gy < (unsigned)p.H;
            const unsigned off = (unsigned)((c * p.H + gy) * p.W + gx) * 4u;
            st.xlo[i] = buf_load(xrs, (in && (unsigned)gx < (unsigned)p.W) ? off : BAD_OFFSET);
            st.xhi[i] = buf_load(xrs, (in && (unsigned)(gx + 1) < (unsigned)p.W) ? off + 4u : BAD_OFFSET);
        }
    };
    auto park = [&](const W2Stage& st, float (&bs)[W2_NGQ], int buf) {
        unsigned char* gzh = w2l + buf * W2_BUF;
        unsigned char* gzl = gzh + W2_GZ;
        unsigned char* xph = gzl + W2_GZ;
        unsigned char* xpl = xph + W2_X;
#pragma unroll
        for (int i = 0; i < W2_NGQ; ++i) {
            const int q = pt + i * 256;
            const float4 f = __builtin_bit_cast(float4, st.gq[i]);
            bs[i] += (f.x + f.y) + (f.z + f.w);
            uint2 vh, vl;
            split_pair(f.x * gscale, f.y * gscale, 1.0f, vh.x, vl.x);
            split_pair(f.z * gscale, f.w * gscale, 1.0f, vh.y, vl.y);
            *reinterpret_cast<uint2*>(gzh + (q >> 4) * W2_GP + (q & 15) * 8) = vh;
            *reinterpret_cast<uint2*>(gzl + (q >> 4) * W2_GP + (q & 15) * 8) = vl;
        }
#pragma unroll
        for (int i = 0; i < W2_NXP; ++i) {
            const int e = pt + i * 256;
            const int c = e / ((W2_TH + 2) * BX_PAIRS), rem = e - c * ((W2_TH + 2) * BX_PAIRS);
            const int r = rem / BX_PAIRS, pr = rem - r * BX_PAIRS;
            unsigned vh, vl;
            split_pair(st.xlo[i], st.xhi[i], 2048.0f, vh, vl);
            *reinterpret_cast<unsigned*>(xph + c * W2_XP + r * BX_ROW + pr * 4) = vh;
            *reinterpret_cast<unsigned*>(xpl + c * W2_XP + r * BX_ROW + pr * 4) = vl;
        }
    };
    auto compute = [&](f32x16 (&acc)[9], int buf) {
        const unsigned char* gzh = w2l + buf * W2_BUF;
        const unsigned char* gzl = gzh + W2_GZ;
        const unsigned char* xph = gzl + W2_GZ;
        const unsigned char* xpl = xph + W2_X;
        const int ga = (m * 32 + j) * W2_GP + kh * 16;
        const int xb = (nn * 32 + j) * W2_XP + kh * 16;
#pragma unroll
        for (int ry = 0; ry < W2_TH; ++ry) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {                                   // k-step = 16 pixels of the row: columns 16 ks + 8 kh ..
                const wf16x8 ah = __builtin_bit_cast(wf16x8, *reinterpret_cast<const u32x4*>(gzh + ga + (ry * 32 + ks * 16) * 2));
                const wf16x8 al = __builtin_bit_cast(wf16x8, *reinterpret_cast<const u32x4*>(gzl + ga + (ry * 32 + ks * 16) * 2));
                const wf16x8 as = ah * (_Float16)0.00048828125f;              // gz_hi 2^-11: partner of the scaled x_lo'
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int row = xb + (ry + dy) * BX_ROW + ks * 32;
                    const u32x4 dh = *reinterpret_cast<const u32x4*>(xph + row);
                    const unsigned dh4 = *reinterpret_cast<const unsigned*>(xph + row + 16);
                    const u32x4 dl = *reinterpret_cast<const u32x4*>(xpl + row);
                    const unsigned dl4 = *reinterpret_cast<const unsigned*>(xpl + row + 16);
                    u32x4 h1, h2, l1, l2;
                    h1.x = __builtin_amdgcn_alignbit(dh.y, dh.x, 16); h1.y = __builtin_amdgcn_alignbit(dh.z, dh.y, 16);
                    h1.z = __builtin_amdgcn_alignbit(dh.w, dh.z, 16); h1.w = __builtin_amdgcn_alignbit(dh4, dh.w, 16);
                    h2.x = dh.y; h2.y = dh.z; h2.z = dh.w; h2.w = dh4;
                    l1.x = __builtin_amdgcn_alignbit(dl.y, dl.x, 16); l1.y = __builtin_amdgcn_alignbit(dl.z, dl.y, 16);
                    l1.z = __builtin_amdgcn_alignbit(dl.w, dl.z, 16); l1.w = __builtin_amdgcn_alignbit(dl4, dl.w, 16);
                    l2.x = dl.y; l2.y = dl.z; l2.z = dl.w; l2.w = dl4;
#define ISR_WS3(T, BH, BL)                                                                                              \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, __builtin_bit_cast(wf16x8, BH), acc[T], 0, 0, 0);   \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(as, __builtin_bit_cast(wf16x8, BL), acc[T], 0, 0, 0);   \
                    acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, __builtin_bit_cast(wf16x8, BH), acc[T], 0, 0, 0);
                    ISR_WS3(dy * 3 + 0, dh, dl)
                    ISR_WS3(dy * 3 + 1, h1, l1)
                    ISR_WS3(dy * 3 + 2, h2, l2)
#undef ISR_WS3
                }
                __builtin_amdgcn_sched_barrier(0);                             // operands are fetched one k-step ahead at most (256 registers)
            }
        }
    };

    // half-tile `it` is computed from buffer it & 1 while the staging waves park half-tile it + 1 (requested one iteration ago) into
    // the other buffer and then request half-tile it + 2: ONE register set, the requests fly while the staging waves wait at the
    // barrier for the MFMAs.  The two roles are separate loops (same number of barriers in each: nhalf + 1), so that the register
    // allocation is the larger of the two roles and not their sum.
    if (consumer) {
        f32x16 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
        __syncthreads();
        for (int it = 0; it < nhalf; ++it) {
            if (!(p.dbg & 1)) compute(acc, it & 1);
            __syncthreads();
        }
        float* slab = p.slabs + (size_t)g * 9 * 64 * 64;
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = m * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
                slab[((size_t)t * 64 + co) * 64 + nn * 32 + j] = acc[t][i];
            }
    } else {
        // one register set (a second one, requests two iterations ahead, measured the same: the staging waves are bound by their
        // own work -- 900 vector instructions and 38 memory requests per thread and half-tile -- not by the latency)
        W2Stage st;
        float bs[W2_NGQ];                                                      // fp32 sums of gz (channel pt / 16 + 16 i)
#pragma unroll
        for (int i = 0; i < W2_NGQ; ++i) bs[i] = 0.0f;
        const bool doPark = !(p.dbg & 2), doFetch = !(p.dbg & 4);
        if (nhalf > 0) {
            fetch(st, 0);
            park(st, bs, 0);
            fetch(st, 1);                                                      // nhalf is even
        }
        __syncthreads();
        for (int it = 0; it < nhalf; ++it) {
            if (it + 1 < nhalf) {
                if (doPark) park(st, bs, (it + 1) & 1);
                if (it + 2 < nhalf && doFetch) fetch(st, it + 2);
            }
            __syncthreads();
        }
        // bias gradient from the fp32 values: staging thread t's sum i belongs to channel t / 16 + 16 i; reduce over the 16 lanes
        if (p.bslabs) {
#pragma unroll
            for (int i = 0; i < W2_NGQ; ++i) {
                float v = bs[i];
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                if ((lane & 15) == 0) p.bslabs[(size_t)g * 64 + (pt >> 4) + 16 * i] = v;
            }
        }
    }
}

// max |gz| over the tensors of a launch: one partial per workgroup, then { 2^S, 2^-S } with max |gz| 2^S in [2^13, 2^14)
struct AbsMaxParams { const float* t[WG_MAX_SEG]; int segments; long long count; };
__global__ __launch_bounds__(256) void wgrad_absmax_kernel(const AbsMaxParams p, float* __restrict__ partial)
{
    __shared__ float red[256];
    float mx = 0.0f;
    const long long quads = p.count >> 2;
    for (int s = 0; s < p.segments; ++s) {
        const float4* src = reinterpret_cast<const float4*>(p.t[s]);
        for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < quads; q += (long long)gridDim.x * 256) {
            const float4 f = src[q];
            mx = fmaxf(fmaxf(mx, fmaxf(fabsf(f.x), fabsf(f.y))), fmaxf(fabsf(f.z), fabsf(f.w)));
        }
        if (blockIdx.x == 0 && threadIdx.x < (p.count & 3)) mx = fmaxf(mx, fabsf(p.t[s][(quads << 2) + threadIdx.x]));
    }
    red[threadIdx.x] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void wgrad_scale_kernel(const float* __restrict__ partial, int n, float* __restrict__ scale)
{
    float mx = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) mx = isr_max(mx, partial[i]);
    mx = isr_block_max(mx);
    if (threadIdx.x == 0) isr_scale_pair(isr_scale_exponent(mx), scale);
}

// ... the same pair from maxima the PRODUCERS of the gz tensors left behind (bit patterns of max |gz|, one word per tensor: the
// split-operand convolutions note it in their epilogues -- SplitConvParams::absmax, Block2Params::zmax / ymax): no pass over gz
struct MaxFlagParams { const unsigned* f[WG_MAX_SEG]; int segments, words; };
__global__ __launch_bounds__(1024) void wgrad_scale_flags_kernel(const MaxFlagParams p, float* __restrict__ scale)
{
    unsigned m = 0u;
    for (int i = threadIdx.x; i < p.words; i += 1024) {
#pragma unroll 8
        for (int s = 0; s < p.segments; ++s) m = isr_max(m, p.f[s][i]);
    }
    m = isr_block_max(m);
    if (threadIdx.x == 0) isr_scale_pair(isr_scale_exponent(__builtin_bit_cast(float, m)), scale);
}

// dw[co][ci][tap] = sum over the G slabs, in a fixed order (bitwise reproducible run to run).  A workgroup owns 64
// consecutive slab elements; its four waves take the slabs g % 4 == wave with four loads in flight each and the
// four partial sums are combined through LDS -- 576 workgroups x 16 independent loads instead of 144 x 8, the
// reduction of 256 slabs (38 MB) is latency bound otherwise.  Workgroup 576 reduces the 64 bias sums the same way.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, int G, float* __restrict__ dw,
                                    int Cout, int Cin, int co0, int ci0, const float* __restrict__ bslabs, float* __restrict__ db,
                                    const float* __restrict__ scale = nullptr,      // split kernel: slabs hold sums scaled by scale[0]
                                    int accumulate = 0)                             // bit 0: dw += (bit 1: db +=) instead of = : straight into .grad
{
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const bool isBias = blockIdx.x == 9 * 64;
    if (isBias && !bslabs) return;
    const size_t stride = isBias ? 64 : (size_t)9 * 64 * 64;
    const float* src = (isBias ? bslabs : slabs + (size_t)blockIdx.x * 64) + lane;
    float s[4] = { 0.f, 0.f, 0.f, 0.f };
    int g = q;
    for (; g + 12 < G; g += 16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += src[(size_t)(g + 4 * k) * stride];
    }
    for (int k = 0; g < G; g += 4, ++k) s[k] += src[(size_t)g * stride];
    part[q][lane] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (q != 0) return;
    const float total = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    if (isBias) {
        if (co0 + lane < Cout) db[co0 + lane] = (accumulate & 2) ? __fadd_rn(db[co0 + lane], total) : total;
        return;
    }
    const int e = blockIdx.x * 64 + lane;                    // over [9][64][64]
    const int ci = e & 63, co = (e >> 6) & 63, tap = e >> 12;
    if (co0 + co >= Cout || ci0 + ci >= Cin) return;
    // (product and sum rounded separately: the same bits as this kernel followed by `grad += dw`)
    const float gval = scale ? __fmul_rn(total, scale[1]) : total;
    float* dst = dw + ((size_t)(co0 + co) * Cin + (ci0 + ci)) * 9 + tap;
    *dst = (accumulate & 1) ? __fadd_rn(*dst, gval) : gval;
}

// ---- host side: fill / plan / launch ---------------------------------------------------------------------------
constexpr int WGRAD_MAX_SLABS = 512;
enum class WGradKind { Exact, Bf16, Split };
#ifdef ISR_DIAG
int g_wgrad_split_form = isr_diag_env_int("ISR_WGRAD_FORM", 2) == 1 ? 1 : 2;   // split kind: 2 = staging on its own waves (the default), 1 = one wave per SIMD
#else
constexpr int g_wgrad_split_form = 2;
#endif

// A validated call: the kernels' parameter block (co0 / ci0 / bslabs change per launch), the scale step's blocks, the rest of the workspace
struct WGradCall {
    WGradParams p;
    AbsMaxParams ap; MaxFlagParams mp;              // split kind: the pass over gz or, with mp.words > 0, the producers' maxima
    float* bslabs; float* partial; float* scale;    // behind the slabs: [WGRAD_MAX_SLABS][64] bias slabs, 512 partial maxima, the scale pair
    float* dw; float* db;
};

// THE validation of the weight gradient, and the only place the parameter block, the workspace carve-up and the tile counts are written.
// 0; -1 bad arguments, or a gzs[k] that is not 16-byte aligned on the bf16 and split kinds; -3 W & 3 on those kinds.
int wgrad_fill(WGradKind kind, const float* const* xs, const float* const* gzs, const void* const* gzmax, int maxWords, int segments,
               float* dw, float* db, void* workspace, int N, int Cin, int H, int W, int Cout, WGradCall* c)
{
    if (!xs || !gzs || segments <= 0 || segments > WG_MAX_SEG || !dw || !workspace || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0)
        return -1;
    const bool quads = kind != WGradKind::Exact;                    // these kinds fetch the gz tile as aligned groups of four pixels
    if (quads && (W & 3)) return -3;
    if (gzmax && maxWords <= 0) return -1;
    WGradParams& p = c->p;
    ISR_DIAG_SET(p.dbg, g_conv_dbg);
    for (int k = 0; k < WG_MAX_SEG; ++k) {
        const bool live = k < segments;
        if (live && (!xs[k] || !gzs[k] || (quads && ((uintptr_t)gzs[k] & 15)) || (gzmax && !gzmax[k]))) return -1;
        p.x[k] = live ? xs[k] : nullptr;
        p.gz[k] = c->ap.t[k] = live ? gzs[k] : nullptr;
        c->mp.f[k] = (live && gzmax) ? (const unsigned*)gzmax[k] : nullptr;
    }
    c->ap.segments = c->mp.segments = segments; c->mp.words = gzmax ? maxWords : 0;
    c->ap.count = (long long)N * Cout * H * W;
    p.slabs = (float*)workspace; c->dw = dw; c->db = db;
    c->bslabs = p.slabs + (size_t)WGRAD_MAX_SLABS * 9 * 64 * 64;
    c->partial = c->bslabs + (size_t)WGRAD_MAX_SLABS * 64; c->scale = c->partial + 512;
    p.scale = kind == WGradKind::Split ? c->scale : nullptr;
    p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.tilesX = (W + WG_TW - 1) / WG_TW; p.tilesY = (H + WG_TH - 1) / WG_TH;
    const long long nt = (long long)N * segments * p.tilesX * p.tilesY;
    if (nt > 0x7fffffffLL) return -1;
    p.ntiles = (int)nt;
    // buffer descriptors address the (at most 64) channels of one image with 32-bit byte offsets
    if ((long long)(Cin < 64 ? Cin : 64) * H * W * 4 > 0x7fffffffLL || (long long)(Cout < 64 ? Cout : 64) * H * W * 4 > 0x7fffffffLL) return -1;
    return 0;
}

// Which kernel the launch of one 64 x 64 channel block takes (coutLeft = Cout - co0), on which grid, and how many slabs it leaves for
// the reduction.  One slab per workgroup; with many tiles one workgroup per CU (fewer slabs to reduce, same balance).
struct WGradPlan { void (*kernel)(WGradParams); int grid, slabs, block, lds; };

WGradPlan wgrad_plan(WGradKind kind, const WGradParams& p, int coutLeft, int splitForm)
{
    const int many = kind == WGradKind::Exact ? 1024 : 512;
    const int G = p.ntiles >= many ? 256 : (p.ntiles < WGRAD_MAX_SLABS ? p.ntiles : WGRAD_MAX_SLABS);
    if (kind == WGradKind::Bf16) return { conv3x3_wgrad_bf16_kernel, G, G, NTHREADS, 0 };
    if (kind == WGradKind::Split) {
#ifdef ISR_DIAG
        if (splitForm == 1) return { conv3x3_wgrad_split_kernel, G, G, NTHREADS, WS_LDS_BYTES };
#endif
        return { conv3x3_wgrad_split2_kernel, G, G, W2_THREADS, W2_LDS_BYTES };
    }
    if (G <= 192) return { conv3x3_wgrad_kernel<3>, 3 * G, G, NTHREADS, 0 };      // few tiles: one workgroup per row of the 3x3
    if (coutLeft <= 32 && G <= WGRAD_MAX_SLABS / 2) return { conv3x3_wgrad_kernel<9, true>, G, 2 * G, NTHREADS, 0 };
    return { conv3x3_wgrad_kernel<9>, G, G, NTHREADS, 0 };
}

// The scale step of the split kind, then per 64 x 64 channel block the kernel and the reduction of its slabs (accumulate: bit 0 dw +=, bit 1 db +=)
int wgrad_launch(WGradKind kind, WGradCall& c, int accumulate, hipStream_t s)
{
    WGradParams& p = c.p; int rc = 0;
    if (kind == WGradKind::Split) {
#ifdef ISR_DIAG
        isr_lds_opt_in<conv3x3_wgrad_split_kernel>(WS_LDS_BYTES);
#endif
        isr_lds_opt_in<conv3x3_wgrad_split2_kernel>(W2_LDS_BYTES);
        if (c.mp.words > 0) rc = isr_launch(wgrad_scale_flags_kernel, dim3(1), dim3(1024), 0, s, nullptr, nullptr, c.mp, c.scale);
        else {
            const long long quads = c.ap.count >> 2;
            const int AB = (int)(quads < 512LL * 256 ? (quads + 255) / 256 > 0 ? (quads + 255) / 256 : 1 : 512);
            rc = isr_launch(wgrad_absmax_kernel, dim3(AB), dim3(256), 0, s, nullptr, nullptr, c.ap, c.partial);
            if (!rc) rc = isr_launch(wgrad_scale_kernel, dim3(1), dim3(256), 0, s, nullptr, nullptr, (const float*)c.partial, AB, c.scale);
        }
    }
    for (int co0 = 0; co0 < p.Cout && !rc; co0 += 64)
        for (int ci0 = 0; ci0 < p.Cin && !rc; ci0 += 64) {
            p.co0 = co0; p.ci0 = ci0;
            p.bslabs = (c.db && ci0 == 0) ? c.bslabs : nullptr;
            const WGradPlan plan = wgrad_plan(kind, p, p.Cout - co0, g_wgrad_split_form);
            const double flops = 2.0 * 9 * (p.Cin - ci0 < 64 ? p.Cin - ci0 : 64) * (p.Cout - co0 < 64 ? p.Cout - co0 : 64) * (double)c.ap.segments * p.N * p.H * p.W;
            // (the split kernels are recorded when profiling is on: the training bench line's weight-gradient family)
            if (kind == WGradKind::Split) rc = isr_launch(ISR_VARIANT_WGRAD_SPLIT, flops, plan.kernel, dim3(plan.grid), dim3(plan.block), plan.lds, s, p);
            else rc = isr_launch(plan.kernel, dim3(plan.grid), dim3(plan.block), plan.lds, s, nullptr, nullptr, p);
            if (!rc) rc = isr_launch(wgrad_reduce_kernel, dim3(9 * 64 + 1), dim3(256), 0, s, nullptr, nullptr, (const float*)p.slabs, plan.slabs,
                                     c.dw, p.Cout, p.Cin, co0, ci0, (const float*)p.bslabs, c.db, p.scale, accumulate);
        }
    return rc;
}

int wgrad(WGradKind kind, const float* const* xs, const float* const* gzs, const void* const* gzmax, int maxWords, int segments,
          float* dw, float* db, int accumulate, void* workspace, int N, int Cin, int H, int W, int Cout, void* stream)
{
    WGradCall c;
    const int rc = wgrad_fill(kind, xs, gzs, gzmax, maxWords, segments, dw, db, workspace, N, Cin, H, W, Cout, &c);
    return rc ? rc : wgrad_launch(kind, c, accumulate & 3, (hipStream_t)stream);
}

}  // namespace

extern "C" {

#ifdef ISR_DIAG
void isrDebugSetWgradSplitForm(int form) { g_wgrad_split_form = form == 1 ? 1 : 2; }
int isrDebugWgradSplitForm(void) { return g_wgrad_split_form; }
#endif

long long isrConvWeightGradWorkspace(int, int, int, int, int)
{
    return (long long)WGRAD_MAX_SLABS * (9 * 64 * 64 + 64) * sizeof(float) + 4096;     // + partial maxima and the scale pair of the split kernel
}

int isrConvWeightGradMaxSegments(void) { return WG_MAX_SEG; }

int isrConv3x3WeightGradSegments(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                 int N, int Cin, int H, int W, int Cout, void* stream)
{
    return wgrad(WGradKind::Exact, xs, gzs, nullptr, 0, segments, dw, db, 0, workspace, N, Cin, H, W, Cout, stream);
}

int isrConv3x3WeightGradSegmentsBf16(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                     int N, int Cin, int H, int W, int Cout, void* stream)
{
    return wgrad(WGradKind::Bf16, xs, gzs, nullptr, 0, segments, dw, db, 0, workspace, N, Cin, H, W, Cout, stream);
}

int isrConv3x3WeightGradSegmentsSplit(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                      int N, int Cin, int H, int W, int Cout, void* stream)
{
    return wgrad(WGradKind::Split, xs, gzs, nullptr, 0, segments, dw, db, 0, workspace, N, Cin, H, W, Cout, stream);
}

int isrConv3x3WeightGradSegmentsSplitMax(const float* const* xs, const float* const* gzs, const void* const* gzmax, int maxWords, int segments,
                                         float* dw, float* db, int accumulate, void* workspace, int N, int Cin, int H, int W, int Cout, void* stream)
{
    return wgrad(WGradKind::Split, xs, gzs, gzmax, maxWords, segments, dw, db, accumulate, workspace, N, Cin, H, W, Cout, stream);
}

int isrConv3x3WeightGrad(const float* x, const float* gz, float* dw, float* db, void* workspace,
                         int N, int Cin, int H, int W, int Cout, void* stream)
{
    return wgrad(WGradKind::Exact, &x, &gz, nullptr, 0, 1, dw, db, 0, workspace, N, Cin, H, W, Cout, stream);
}

}  // extern "C"
