// STRIDE-2 3x3 convolution, y = act(conv2d(x, w, b, stride = 2, padding = 1)): the layer with which the reference's discriminators
// (SuperresolutionNetwork/losses/enhancenetsmall.py, enhancenetlarge.py) halve the image from 128 x 128 to 4 x 4, with 16 .. 256
// channels.  Forward, data gradient and weight gradient, all in exact fp32 MFMA (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain),
// every sum in a fixed order: the same bits on every run.
//
// x [N][Cin][H][W], w [Cout][Cin][3][3] (as nn.Conv2d holds it), y [N][Cout][H/2][W/2], all packed fp32; H and W even, Cin and Cout
// multiples of 16 up to 256.  Output pixel (i, j) reads input rows 2i - 1 .. 2i + 1: only the TOP row and LEFT column of the image read
// padding (2i + 1 <= H - 1 always).
//
// THE PIXEL DIMENSION IS FLATTENED over the batch: the deepest layers are 8 x 8 -> 4 x 4 with 256 channels, 16 output pixels per image,
// so an MFMA tile of pixels runs over (n, i, j) of the whole launch and a workgroup may span several images.
//
// FORWARD (conv3x3s2_fwd_kernel).  Exactly nine Cin x Cout products per output pixel.  A workgroup owns CT output channels x PT flattened
// pixels (64 x 64, or 32 / 16 channels x 128 pixels for the narrow layers) and walks Cin in chunks of 8: the chunk's operands go to LDS as
// an im2col image X[tap][8 ci][pixel] -- the stride-2 gather happens ONCE, on the way in; in LDS the even / odd input columns of a tap are
// already apart, pixels are contiguous and every fragment read is conflict free (rows padded by 16 floats: lanes l and l + 16 of a
// 32-lane half read rows k and k + 1) -- and W[tap][8 ci][cout].  18 k-steps of 4 per chunk; wave = 2 x 2 blocks of 16 x 16: four
// independent accumulators, which is what the 16x16x4 MFMA needs to issue back to back.  Bias and activation in the epilogue; a lane's
// 16 neighbours write 64 contiguous bytes of one channel.
//
// DATA GRADIENT (conv3x3s2_dgrad_kernel).  gx[n][ci][p][q] = sum_{co, ky, kx : p = 2i + ky - 1, q = 2j + kx - 1} gz[n][co][i][j] w[co][ci][ky][kx],
// decomposed by the parity of the output: row p = 2u + a receives (ky = 1, i = u) for a = 0 and (ky = 2, i = u), (ky = 0, i = u + 1) for a = 1,
// columns alike: four phases of 1, 2, 2 and 4 taps over the same gz pixels (u .. u + 1, v .. v + 1).  Here the BOTTOM row and RIGHT column
// lose a tap (i = H / 2 is outside).  A workgroup owns CT input channels x PT flattened low-resolution pixels x the four phases and walks
// Cout in chunks of 8: G[neighbour][8 co][pixel] and W[tap][8 co][ci] in LDS, nine products per k-step into the phase's accumulators.
// A lane holds both column phases of an output row: 8-byte stores, 16 lanes write 128 contiguous bytes.  w is taken as it is.
//
// WEIGHT GRADIENT (conv3x3s2_wgrad_kernel + conv3x3s2_wgrad_sum_kernel).  dw[co][ci][tap] = sum over the pixels of every segment
// (x_k, gz_k) of gz[co][pixel] x[ci][tap of pixel]; db[co] = sum gz.  The MFMA k dimension is the flattened pixel (segment, n, i, j); a
// workgroup owns 32 co x 32 ci x 9 taps (wave = 16 x 16 x 9: nine accumulators) and ONE SLAB of the pixels, in chunks of 32; the bias
// sum rides along as a tenth product against a fragment of ones (waves of the first ci block only).  The slabs go to the workspace
// and the second kernel adds them in slab order.
#include "sr_conv_common.h"

namespace {

constexpr int ISR_VARIANT_CONV_S2_FWD = 48;          // ops.VARIANT_NAMES
constexpr int ISR_VARIANT_CONV_S2_DGRAD = 49;
constexpr int ISR_VARIANT_CONV_S2_WGRAD = 50;
constexpr int ISR_VARIANT_CONV_S2_WGRAD_SUM = 51;

typedef float s2_f32x4 __attribute__((ext_vector_type(4)));

constexpr int S2_KC = 8;                              // channels of the summed dimension per LDS chunk
constexpr int S2_ROWS = 9 * S2_KC;                    // rows [tap][channel] of a chunk's weight (and im2col) image
// row stride (floats) of an LDS image read as fragments: stride % 32 == 16 puts rows k, k + 1 of a 32-lane half on disjoint banks
constexpr int s2_stride(int n) { return n % 32 == 16 ? n : n + 16; }
constexpr int S2_MAX_C = 256;
constexpr int S2_SEGMENTS = 32;
constexpr int S2_WG_CHUNK = 32;                       // pixels per chunk of the weight gradient
constexpr int S2_WG_STRIDE = S2_WG_CHUNK + 2;         // [channel][pixel] rows: channel c, pixel k on bank (2 c + k) % 32
constexpr int S2_WG_MAX_SLABS = 256;

struct S2Params {
    const float* x; const float* w; const float* bias; float* y;
    int Cin, Cout, H, W, Ho, Wo;
    int pixTiles;
    long long pixels;                                 // N Ho Wo
    int act; float slope;
};

__device__ __forceinline__ s2_f32x4 s2_mfma(float a, float b, s2_f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// waves WR (channels) x WC (pixels), each MA x NB blocks of 16 x 16: CT = 16 WR MA channels, PT = 16 WC NB pixels
template <int WR, int WC, int MA, int NB>
__global__ __launch_bounds__(NTHREADS) void conv3x3s2_fwd_kernel(const S2Params p)
{
    constexpr int CT = WR * MA * 16, PT = WC * NB * 16, WS = s2_stride(CT), XS = s2_stride(PT), RP = NTHREADS / PT;
    static_assert(WR * WC == 4 && NTHREADS % PT == 0 && S2_ROWS % RP == 0, "tile");
    __shared__ float lds[S2_ROWS * (WS + XS)];
    float* const Ws = lds;
    float* const Xs = lds + S2_ROWS * WS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pt = bid % p.pixTiles, co0 = (bid / p.pixTiles) * CT;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo;

    // the pixel this thread stages (the same one in every chunk)
    const int sp = tid % PT, srow = tid / PT;
    const long long SP = (long long)pt * PT + sp;
    const bool svalid = SP < p.pixels;
    const long long sn = svalid ? SP / HoWo : 0;
    const int srem = svalid ? (int)(SP - sn * HoWo) : 0;
    const int iy0 = 2 * (srem / p.Wo) - 1, ix0 = 2 * (srem % p.Wo) - 1;
    const float* const xn = p.x + (size_t)sn * p.Cin * HW;

    s2_f32x4 acc[MA][NB];
#pragma unroll
    for (int m = 0; m < MA; ++m)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[m][n] = s2_f32x4{0.f, 0.f, 0.f, 0.f};

    // a chunk's operands travel global -> registers -> LDS; the NEXT chunk's loads are issued before this chunk's MFMAs and land under them
    constexpr int XQ = S2_ROWS / RP, WQ = (CT * S2_ROWS + NTHREADS - 1) / NTHREADS;
    float xreg[XQ], wreg[WQ];
    auto fetch = [&](int ci0) {
        // im2col image of the chunk: row = tap * 8 + channel, zeros for the padding row / column and beyond the last pixel
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int r = srow + q * RP, tap = r >> 3, cl = r & 7;
            const int iy = iy0 + tap / 3, ix = ix0 + tap % 3;
            const bool ok = svalid && iy >= 0 && ix >= 0;
            xreg[q] = ok ? xn[(size_t)(ci0 + cl) * HW + iy * p.W + ix] : 0.0f;
        }
        // weights of the chunk: per output channel 72 contiguous floats [channel][tap]
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int e = tid + q * NTHREADS;
            const int co = e / S2_ROWS, r = e - co * S2_ROWS;
            wreg[q] = e < CT * S2_ROWS ? p.w[((size_t)(co0 + co) * p.Cin + ci0) * 9 + r] : 0.0f;
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int q = 0; q < XQ; ++q) Xs[(srow + q * RP) * XS + sp] = xreg[q];
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int e = tid + q * NTHREADS;
            const int co = e / S2_ROWS, r = e - co * S2_ROWS, cl = r / 9, tap = r - cl * 9;
            if (e < CT * S2_ROWS) Ws[(tap * S2_KC + cl) * WS + co] = wreg[q];
        }
    };
    fetch(0);
#pragma unroll 1
    for (int ci0 = 0; ci0 < p.Cin; ci0 += S2_KC) {
        park();
        __syncthreads();
        if (ci0 + S2_KC < p.Cin) fetch(ci0 + S2_KC);
#pragma unroll 3
        for (int ks = 0; ks < S2_ROWS / 4; ++ks) {
            const int k = ks * 4 + (lane >> 4);
            float a[MA], b[NB];
#pragma unroll
            for (int m = 0; m < MA; ++m) a[m] = Ws[k * WS + (wr * MA + m) * 16 + (lane & 15)];
#pragma unroll
            for (int n = 0; n < NB; ++n) b[n] = Xs[k * XS + (wc * NB + n) * 16 + (lane & 15)];
#pragma unroll
            for (int m = 0; m < MA; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc[m][n] = s2_mfma(a[m], b[n], acc[m][n]);
        }
        __syncthreads();
    }

    // ---- epilogue: D row (cout) = 4 (lane >> 4) + reg, column (pixel) = lane & 15
    isr_with_act(p.act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const long long P = (long long)pt * PT + (wc * NB + n) * 16 + (lane & 15);
            if (P >= p.pixels) continue;
            const long long in = P / HoWo;
            const int rem = (int)(P - in * HoWo);
#pragma unroll
            for (int m = 0; m < MA; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = co0 + (wr * MA + m) * 16 + 4 * (lane >> 4) + i;
                    const float v = acc[m][n][i] + (p.bias ? p.bias[co] : 0.0f);
                    p.y[((size_t)in * p.Cout + co) * HoWo + rem] = isr_activate<ACT>(v, p.slope);
                }
        }
    });
}

// ---- DATA GRADIENT ----------------------------------------------------------------------------------------------------------------
struct S2GradParams {
    const float* g; const float* w; float* gx;
    int Cin, Cout, H, W, Ho, Wo;
    int pixTiles;
    long long pixels;                                 // N Ho Wo: low-resolution pixels, four output pixels each
};

template <int WR, int WC, int MA, int NB>
__global__ __launch_bounds__(NTHREADS) void conv3x3s2_dgrad_kernel(const S2GradParams p)
{
    constexpr int CT = WR * MA * 16, PT = WC * NB * 16, WS = s2_stride(CT), XS = s2_stride(PT), RP = NTHREADS / PT, GROWS = 4 * S2_KC;
    static_assert(WR * WC == 4 && NTHREADS % PT == 0 && GROWS % RP == 0, "tile");
    __shared__ float lds[S2_ROWS * WS + GROWS * XS];
    float* const Ws = lds;                            // [tap][8 co][ci]
    float* const Gs = lds + S2_ROWS * WS;             // [neighbour 2 di + dj][8 co][pixel]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int pt = bid % p.pixTiles, ci0 = (bid / p.pixTiles) * CT;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo;

    const int sp = tid % PT, srow = tid / PT;
    const long long SP = (long long)pt * PT + sp;
    const bool svalid = SP < p.pixels;
    const long long sn = svalid ? SP / HoWo : 0;
    const int srem = svalid ? (int)(SP - sn * HoWo) : 0;
    const int su = srem / p.Wo, sv = srem % p.Wo;
    const float* const gn = p.g + (size_t)sn * p.Cout * HoWo;

    s2_f32x4 acc[4][MA][NB];                          // [phase 2 a + b]
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int m = 0; m < MA; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) acc[ph][m][n] = s2_f32x4{0.f, 0.f, 0.f, 0.f};

    // (registers between global memory and LDS, the next chunk fetched under this chunk's MFMAs: as the forward kernel)
    constexpr int GQ = GROWS / RP, WQ = (CT * S2_ROWS + NTHREADS - 1) / NTHREADS;
    float greg[GQ], wreg[WQ];
    auto fetch = [&](int co0) {
        // the four neighbours (u + di, v + dj) of the chunk's gradient: zeros below the last row and right of the last column
#pragma unroll
        for (int q = 0; q < GQ; ++q) {
            const int r = srow + q * RP, nb = r >> 3, cl = r & 7;
            const int iy = su + (nb >> 1), ix = sv + (nb & 1);
            const bool ok = svalid && iy < p.Ho && ix < p.Wo;
            greg[q] = ok ? gn[(size_t)(co0 + cl) * HoWo + iy * p.Wo + ix] : 0.0f;
        }
        // weights: per output channel of the chunk CT * 9 contiguous floats [ci][tap]
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int e = tid + q * NTHREADS;
            const int cl = e / (CT * 9), r = e - cl * (CT * 9);
            wreg[q] = e < CT * S2_ROWS ? p.w[((size_t)(co0 + cl) * p.Cin + ci0) * 9 + r] : 0.0f;
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int q = 0; q < GQ; ++q) Gs[(srow + q * RP) * XS + sp] = greg[q];
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int e = tid + q * NTHREADS;
            const int cl = e / (CT * 9), r = e - cl * (CT * 9), ci = r / 9, tap = r - ci * 9;
            if (e < CT * S2_ROWS) Ws[(tap * S2_KC + cl) * WS + ci] = wreg[q];
        }
    };
    fetch(0);
#pragma unroll 1
    for (int co0 = 0; co0 < p.Cout; co0 += S2_KC) {
        park();
        __syncthreads();
        if (co0 + S2_KC < p.Cout) fetch(co0 + S2_KC);
#pragma unroll
        for (int s = 0; s < S2_KC / 4; ++s) {
            const int k = s * 4 + (lane >> 4);
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    float b[NB];
#pragma unroll
                    for (int n = 0; n < NB; ++n) b[n] = Gs[((2 * di + dj) * S2_KC + k) * XS + (wc * NB + n) * 16 + (lane & 15)];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        if ((ky == 0) != (di == 1)) continue;                // di = 0: ky = 1, 2; di = 1: ky = 0
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            if ((kx == 0) != (dj == 1)) continue;
                            const int tap = 3 * ky + kx, ph = 2 * (ky == 1 ? 0 : 1) + (kx == 1 ? 0 : 1);
#pragma unroll
                            for (int m = 0; m < MA; ++m) {
                                const float a = Ws[(tap * S2_KC + k) * WS + (wr * MA + m) * 16 + (lane & 15)];
#pragma unroll
                                for (int n = 0; n < NB; ++n) acc[ph][m][n] = s2_mfma(a, b[n], acc[ph][m][n]);
                            }
                        }
                    }
                }
        }
        __syncthreads();
    }

    // ---- epilogue: D row (ci) = 4 (lane >> 4) + reg, column (pixel) = lane & 15; the lane holds columns 2v, 2v + 1 of rows 2u, 2u + 1
#pragma unroll
    for (int n = 0; n < NB; ++n) {
        const long long P = (long long)pt * PT + (wc * NB + n) * 16 + (lane & 15);
        if (P >= p.pixels) continue;
        const long long in = P / HoWo;
        const int rem = (int)(P - in * HoWo);
        const int u = rem / p.Wo, v = rem % p.Wo;
#pragma unroll
        for (int m = 0; m < MA; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ci = ci0 + (wr * MA + m) * 16 + 4 * (lane >> 4) + i;
                float* const o = p.gx + ((size_t)in * p.Cin + ci) * HW + (size_t)(2 * u) * p.W + 2 * v;
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    float2 t;
                    t.x = acc[2 * a][m][n][i]; t.y = acc[2 * a + 1][m][n][i];
                    *reinterpret_cast<float2*>(o + a * p.W) = t;
                }
            }
    }
}

// ---- WEIGHT GRADIENT ----------------------------------------------------------------------------------------------------------------
struct S2WgradParams {
    const float* xs[S2_SEGMENTS]; const float* gzs[S2_SEGMENTS];
    float* slab;                                      // [slabs][Cout][Cin][9], then [slabs][Cout]
    float* bslab;
    int Cin, Cout, H, W, Ho, Wo;
    int coTiles, ciTiles, slabs, chunksPerSlab;
    long long perSegment, pixels;                     // N Ho Wo and segments N Ho Wo
};

__global__ __launch_bounds__(NTHREADS) void conv3x3s2_wgrad_kernel(const S2WgradParams p)
{
    constexpr int ST = S2_WG_STRIDE;
    __shared__ float lds[32 * ST + 9 * 32 * ST];
    float* const Gs = lds;                            // [32 co][pixel]
    float* const Xs = lds + 32 * ST;                  // [tap][32 ci][pixel]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int tiles = p.coTiles * p.ciTiles;
    const int slab = blockIdx.x / tiles, tile = blockIdx.x - slab * tiles;
    const int co0 = (tile / p.ciTiles) * 32, ci0 = (tile % p.ciTiles) * 32;
    const int HW = p.H * p.W, HoWo = p.Ho * p.Wo;
    const bool active = co0 + wr * 16 < p.Cout && ci0 + wc * 16 < p.Cin;     // (wave uniform: channel counts are multiples of 16)
    const bool withBias = active && ci0 == 0 && wc == 0;

    s2_f32x4 acc[9], accb = s2_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = s2_f32x4{0.f, 0.f, 0.f, 0.f};

    const int sp = tid & 31, srow = tid >> 5;         // this thread stages pixel sp of the chunk, channels srow + 8 q
    const long long chunk0 = (long long)slab * p.chunksPerSlab;
#pragma unroll 1
    for (int c = 0; c < p.chunksPerSlab; ++c) {
        const long long P = (chunk0 + c) * S2_WG_CHUNK + sp;
        if ((chunk0 + c) * S2_WG_CHUNK >= p.pixels) break;                   // (block uniform)
        const bool valid = P < p.pixels;
        const int seg = valid ? (int)(P / p.perSegment) : 0;
        const long long R = valid ? P - (long long)seg * p.perSegment : 0;
        const long long n = R / HoWo;
        const int rem = (int)(R - n * HoWo);
        const int iy0 = 2 * (rem / p.Wo) - 1, ix0 = 2 * (rem % p.Wo) - 1;
        const float* const gn = p.gzs[seg] + (size_t)n * p.Cout * HoWo + rem;
        const float* const xn = p.xs[seg] + (size_t)n * p.Cin * HW;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = srow + 8 * q;
            Gs[ch * ST + sp] = (valid && co0 + ch < p.Cout) ? gn[(size_t)(co0 + ch) * HoWo] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ch = srow + 8 * q;
            const bool okc = valid && ci0 + ch < p.Cin;
            const float* const xc = xn + (size_t)(ci0 + ch) * HW;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = iy0 + tap / 3, ix = ix0 + tap % 3;
                Xs[(tap * 32 + ch) * ST + sp] = (okc && iy >= 0 && ix >= 0) ? xc[iy * p.W + ix] : 0.0f;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll 2
            for (int ks = 0; ks < S2_WG_CHUNK / 4; ++ks) {
                const int k = ks * 4 + (lane >> 4);
                const float a = Gs[(wr * 16 + (lane & 15)) * ST + k];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
                    acc[tap] = s2_mfma(a, Xs[(tap * 32 + wc * 16 + (lane & 15)) * ST + k], acc[tap]);
                if (withBias) accb = s2_mfma(a, 1.0f, accb);
            }
        }
        __syncthreads();
    }

    // ---- the slab: D row (co) = 4 (lane >> 4) + reg, column (ci) = lane & 15
    if (!active) return;
    float* const out = p.slab + (size_t)slab * p.Cout * p.Cin * 9;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int co = co0 + wr * 16 + 4 * (lane >> 4) + i, ci = ci0 + wc * 16 + (lane & 15);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) out[((size_t)co * p.Cin + ci) * 9 + tap] = acc[tap][i];
        if (withBias && (lane & 15) == 0) p.bslab[(size_t)slab * p.Cout + co] = accb[i];
    }
}

// dw / db = the slabs added in slab order
__global__ __launch_bounds__(NTHREADS) void conv3x3s2_wgrad_sum_kernel(const float* slab, const float* bslab, float* dw, float* db,
                                                                       int wcount, int cout, int slabs)
{
    const int e = blockIdx.x * NTHREADS + threadIdx.x;
    if (e < wcount) {
        float s = 0.0f;
        for (int k = 0; k < slabs; ++k) s += slab[(size_t)k * wcount + e];
        dw[e] = s;
    } else if (e < wcount + cout && db) {
        float s = 0.0f;
        for (int k = 0; k < slabs; ++k) s += bslab[(size_t)k * cout + (e - wcount)];
        db[e - wcount] = s;
    }
}

bool s2_supported(long long N, int Cin, int Cout, int H, int W)
{
    if (N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || H > 16384 || W > 16384) return false;
    if (Cin < 16 || Cout < 16 || Cin > S2_MAX_C || Cout > S2_MAX_C || (Cin & 15) || (Cout & 15)) return false;
    // flattened pixels and every tensor's element count stay well inside 32-bit tile arithmetic
    const long long px = N * (H / 2) * (W / 2);
    return px <= 0x3fffffffLL && N * (long long)S2_MAX_C * H * W <= (1LL << 40);
}

int s2_wgrad_tiles(int Cin, int Cout) { return ((Cout + 31) / 32) * ((Cin + 31) / 32); }

int s2_wgrad_max_slabs(int Cin, int Cout)
{
    const int s = 1024 / s2_wgrad_tiles(Cin, Cout);                          // about four workgroups per CU
    return s < 1 ? 1 : (s > S2_WG_MAX_SLABS ? S2_WG_MAX_SLABS : s);
}

// the tile of a layer with C channels on the MFMA row dimension: 64 x 64, or 128 pixels x 32 / 16 channels
template <typename P, typename F64, typename F32, typename F16>
int s2_launch_tiled(int variant, double flops, int C, P& p, hipStream_t stream, F64 k64, F32 k32, F16 k16)
{
    const int CT = (C % 64 == 0) ? 64 : (C % 32 == 0) ? 32 : 16, PT = CT == 64 ? 64 : 128;
    p.pixTiles = (int)((p.pixels + PT - 1) / PT);
    const long long grid = (long long)p.pixTiles * (C / CT);
    if (grid > 0x3fffffffLL) return -3;
    if (CT == 64) return isr_launch(variant, flops, k64, dim3((unsigned)grid), dim3(NTHREADS), 0, stream, p);
    if (CT == 32) return isr_launch(variant, flops, k32, dim3((unsigned)grid), dim3(NTHREADS), 0, stream, p);
    return isr_launch(variant, flops, k16, dim3((unsigned)grid), dim3(NTHREADS), 0, stream, p);
}

} // namespace

extern "C" {

int isrConv3x3S2Supported(int N, int Cin, int Cout, int H, int W)
{
    return s2_supported(N, Cin, Cout, H, W) ? 1 : 0;
}

int isrConv3x3S2Forward(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W, int Cout,
                        int act, float slope, void* stream)
{
    if (!x || !w || !y) return -1;
    if (act != ISR_ACT_NONE && act != ISR_ACT_LEAKY) return -1;
    if (!s2_supported(N, Cin, Cout, H, W)) return -3;
    S2Params p;
    p.x = x; p.w = w; p.bias = bias; p.y = y;
    p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
    p.pixels = (long long)N * p.Ho * p.Wo;
    p.act = act; p.slope = slope;
    const double flops = 2.0 * 9 * Cin * Cout * (double)p.pixels;
    return s2_launch_tiled(ISR_VARIANT_CONV_S2_FWD, flops, Cout, p, (hipStream_t)stream, conv3x3s2_fwd_kernel<2, 2, 2, 2>,
                           conv3x3s2_fwd_kernel<1, 4, 2, 2>, conv3x3s2_fwd_kernel<1, 4, 1, 2>);
}

int isrConv3x3S2DataGrad(const float* gz, const float* w, float* gx, int N, int Cin, int H, int W, int Cout, void* stream)
{
    if (!gz || !w || !gx || ((uintptr_t)gx & 7)) return -1;
    if (!s2_supported(N, Cin, Cout, H, W)) return -3;
    S2GradParams p;
    p.g = gz; p.w = w; p.gx = gx;
    p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
    p.pixels = (long long)N * p.Ho * p.Wo;
    const double flops = 2.0 * 9 * Cin * Cout * (double)p.pixels;
    return s2_launch_tiled(ISR_VARIANT_CONV_S2_DGRAD, flops, Cin, p, (hipStream_t)stream, conv3x3s2_dgrad_kernel<2, 2, 2, 2>,
                           conv3x3s2_dgrad_kernel<1, 4, 2, 2>, conv3x3s2_dgrad_kernel<1, 4, 1, 2>);
}

long long isrConv3x3S2WeightGradWorkspace(int N, int Cin, int H, int W, int Cout)
{
    if (!s2_supported(N, Cin, Cout, H, W)) return 0;
    return (long long)s2_wgrad_max_slabs(Cin, Cout) * ((long long)Cout * Cin * 9 + Cout) * 4;
}

int isrConv3x3S2WeightGradSegments(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                   int N, int Cin, int H, int W, int Cout, void* stream)
{
    if (!xs || !gzs || !dw || !workspace || segments <= 0 || segments > S2_SEGMENTS || segments > isrConvWeightGradMaxSegments()) return -1;
    if (!s2_supported((long long)N * segments, Cin, Cout, H, W)) return -3;
    S2WgradParams p;
    for (int k = 0; k < S2_SEGMENTS; ++k) {
        p.xs[k] = xs[k < segments ? k : 0]; p.gzs[k] = gzs[k < segments ? k : 0];
        if (!p.xs[k] || !p.gzs[k]) return -1;
    }
    p.Cin = Cin; p.Cout = Cout; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2;
    p.perSegment = (long long)N * p.Ho * p.Wo;
    p.pixels = p.perSegment * segments;
    p.coTiles = (Cout + 31) / 32; p.ciTiles = (Cin + 31) / 32;
    const long long chunks = (p.pixels + S2_WG_CHUNK - 1) / S2_WG_CHUNK;
    const int most = s2_wgrad_max_slabs(Cin, Cout);
    p.slabs = (int)(chunks < most ? chunks : most);
    p.chunksPerSlab = (int)((chunks + p.slabs - 1) / p.slabs);
    p.slabs = (int)((chunks + p.chunksPerSlab - 1) / p.chunksPerSlab);       // no empty slab: every slab word is written before it is read
    const int wcount = Cout * Cin * 9;
    p.slab = (float*)workspace;
    p.bslab = p.slab + (size_t)most * wcount;
    const double flops = 2.0 * 9 * Cin * Cout * (double)p.pixels;
    const int rc = isr_launch(ISR_VARIANT_CONV_S2_WGRAD, flops, conv3x3s2_wgrad_kernel, dim3((unsigned)(p.coTiles * p.ciTiles * p.slabs)),
                              dim3(NTHREADS), 0, (hipStream_t)stream, p);
    if (rc != 0) return rc;
    return isr_launch(ISR_VARIANT_CONV_S2_WGRAD_SUM, 0.0, conv3x3s2_wgrad_sum_kernel, dim3((unsigned)((wcount + Cout + NTHREADS - 1) / NTHREADS)),
                      dim3(NTHREADS), 0, (hipStream_t)stream, (const float*)p.slab, (const float*)p.bslab, dw, db, wcount, Cout, p.slabs);
}

} // extern "C"
