// SPLIT-OPERAND transposed convolution: ConvTranspose2d(64, 64, 3, stride = 2, padding = 1, output_padding = 1), the learned x2
// upsampling of the TecoGAN generator (SuperresolutionNetwork/models/tecogan.py:55-59), with bias and activation in the epilogue.
//
// PHASE DECOMPOSITION.  The weight is w[ci][co][ky][kx], the output 2h x 2w, and an output pixel (2i + a, 2j + b) receives
// x[i + di][j + dj] w[ky][kx] for the taps with 2 (i + di) - 1 + ky = 2 i + a:
//     a = 0: (ky = 1, di = 0)                      a = 1: (ky = 2, di = 0), (ky = 0, di = 1)          (columns alike in kx, dj, b)
// so the four phases (a, b) are four channel-mixing sums of 1, 2, 2 and 4 taps over the SAME low-resolution pixels (i .. i + 1,
// j .. j + 1): nine 64 x 64 products per low-resolution pixel for its four output pixels -- 2.25 taps per output pixel, no zero
// stuffing, no multiply by a structural zero.  Input rows >= h and columns >= w contribute nothing (output_padding = 1 puts
// the missing neighbour outside the image).
//
// Arithmetic: the split-operand scheme of sr_conv_split.hip (sr_split_common.h): activations as (hi, lo' = lo 2^11) fp16 pairs made on
// the way into LDS, weights as scaled (hi, lo) pairs prepared once (sr_split_prepare.hip), three v_mfma_f32_32x32x16_f16 per product, fp32 accumulation.
//
// Structure: workgroup = 4 x 32 low-resolution pixels (8 x 64 output pixels) x 64 output channels, 4 waves, wave w owns low-resolution
// row w: FOUR accumulator sets (the phases) x 2 channel blocks = 128 registers.  The input is staged in chunks of 32 channels as
// LDS[hi | lo'][group of 8 channels][5 x 33 patch pixels] -- the tile plus one halo row below and one halo column to the right, zero
// outside the image -- and the weights [hi | lo][tap][lane half][cout] of one 16-channel k-step pass through LDS, fetched into registers
// under the previous k-step's MFMAs (as conv3x3_split_kernel).  Per k-step the wave reads the four neighbour fragments once and walks
// the nine taps grouped by neighbour.  58 KB of LDS: two workgroups per CU.
//
// Stores.  By bytes the layer IS its store (the second layer of a 1080p frame writes 531 MB).  In the MFMA result a lane holds the
// two phases b = 0, 1 of one output row: 8 contiguous bytes of a channel.  Neighbouring lanes (j, j ^ 1) trade halves of a channel pair
// in registers (one DPP move each), after which the even lane holds four consecutive pixels of channel c and the odd lane the same four
// of channel c + 1: one 16-byte store per lane, a wave instruction writes four runs of 256 contiguous bytes.  (w odd, or planes that
// are not 16-byte aligned: dword stores.)
//
// Training: the same kernel over a whole batch in one launch (convt3x3s2_split_kernel<true>), and the DATA GRADIENT
// (convt3x3s2_dgrad_split_kernel, below) over the phase-major output gradient that isrConvTransposePhaseGradient (sr_train.hip) writes.
#include "sr_split_common.h"

namespace {

constexpr int ISR_VARIANT_CONVT_SPLIT = 37;                                  // convt3x3s2_split_kernel (ops.VARIANT_NAMES)
constexpr int CT_H = 4, CT_W = 32;                                           // low-resolution tile
constexpr int CP_H = CT_H + 1, CP_W = CT_W + 1, CP_PIX = CP_H * CP_W;        // 165 patch pixels
constexpr int CT_PART = S_GROUPS * CP_PIX;                                   // units of the hi (or lo') patch of a 32-channel chunk: 660
constexpr int CT_PUNITS = 2 * CT_PART;
constexpr int CT_LDS_BYTES = (CT_PUNITS + S_WUNITS) * 16;                    // 21 120 + 36 864 = 57 984: two workgroups per CU
constexpr int CT_C = 64;                                                     // channels in and out
constexpr int CT_KSTEPS = CT_C / 16;

struct ConvTParams {
    const float* x; const u32x4* wq; const float* bias; float* y;
    int h, w;                         // INPUT (low-resolution) size; the output is 2h x 2w
    int xPlane, yPlane;
    int tilesX, tilesY;
    int act; float slope;
    int wide;                         // 1: w even, yPlane % 4 == 0, y 16-byte aligned -- the 16-byte stores
    unsigned* absmax;                 // range guard (may be NULL), as SplitConvParams::absmax
    int tilesImage;                   // BATCH form (training: N images in one launch): tiles per image, floats between images
    long long xImage, yImage;
};

// the neighbour lane's value (lane ^ 1): DPP quad_perm [1, 0, 3, 2]
__device__ __forceinline__ float ct_swap1(float v)
{
    const int i = __builtin_bit_cast(int, v);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false));
}

// BATCH: the grid covers N images (image bid / tilesImage, tile bid % tilesImage) -- the training forward: one launch per frame of a batch of
// clips, not one per clip
template <bool BATCH>
__global__ __launch_bounds__(S_THREADS, 2) void convt3x3s2_split_kernel(const ConvTParams p)
{
    extern __shared__ u32x4 patch[];                                         // CT_PUNITS patch units, then the weight buffer
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hh = lane >> 5;
    int bid;
    {   // an XCD (= an L2) gets a contiguous range of tiles
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
    }
    const float* xbase = p.x;
    float* ybase = p.y;
    if constexpr (BATCH) {
        const int n = bid / p.tilesImage;
        bid -= n * p.tilesImage;
        xbase += (size_t)n * p.xImage;
        ybase += (size_t)n * p.yImage;
    }
    const int tx = bid % p.tilesX, ty = bid / p.tilesX;
    const int oy0 = ty * CT_H, ox0 = tx * CT_W;                              // low-resolution origin of the tile

    const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xbase), 0, (int)((size_t)CT_C * p.xPlane * 4), 0x00020000);
    const unsigned planeBytes = (unsigned)p.xPlane * 4u;
    u32x4* const wbuf = patch + CT_PUNITS;

    f32x16 acc[4][2];                                                        // [phase 2 a + b][channel block]
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ph][cb][i] = 0.0f;

    // weights of k-step ks: 2304 units [part][tap][lane half][64 couts]; thread t moves unit (tap i, part t / 128, t % 128), i = 0 .. 8:
    // byte 16 t + 4096 (4 i + ks) of the prepared image
    const rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(p.wq + 1), 0, 9 * CT_KSTEPS * 4096, 0x00020000);
    u32x4* const wdst = wbuf + (tid >> 7) * S_WPART + (tid & 127);
    u32x4 wreg[9];
    auto wfetch = [&](int ks) {
        if (ks >= CT_KSTEPS) return;
#pragma unroll
        for (int i = 0; i < 9; ++i) wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(wrs, tid * 16, (i * CT_KSTEPS + ks) * 4096, 0);
    };
    auto wpark = [&]() {
#pragma unroll
        for (int i = 0; i < 9; ++i) wdst[i * 128] = wreg[i];
    };
    wfetch(0);                                                               // in flight under the first staging

#pragma unroll 1
    for (int cin0 = 0; cin0 < CT_C; cin0 += S_CHUNK) {
        // ---- stage the 32-channel patch, split into hi and lo' parts: unit = (channel group g, patch pixel); rows oy0 .. oy0 + 4, columns
        //      ox0 .. ox0 + 32, zeros beyond the image (the buffer load of the out-of-range offset returns 0)
        for (int u0 = tid; u0 < CT_PART; u0 += 3 * S_THREADS) {
            float v[3][8];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int u = u0 + k * S_THREADS;
                const int g = u / CP_PIX, pix = u - g * CP_PIX;
                const int r = pix / CP_W, c = pix - r * CP_W;
                const int iy = oy0 + r, ix = ox0 + c;
                const bool ok = u < CT_PART && iy < p.h && ix < p.w;
                const unsigned base = (unsigned)(cin0 + g * 8) * planeBytes + (unsigned)(iy * p.w + ix) * 4u;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] = buf_load(xrs, ok ? base + (unsigned)e * planeBytes : BAD_OFFSET);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int u = u0 + k * S_THREADS;
                f16x8 qh, ql;
#pragma unroll
                for (int e = 0; e < 8; ++e) { _Float16 a, b; split16x(v[k][e], a, b); qh[e] = a; ql[e] = b; }
                if (u < CT_PART) { patch[u] = __builtin_bit_cast(u32x4, qh); patch[CT_PART + u] = __builtin_bit_cast(u32x4, ql); }
            }
        }
        wpark();                                                             // k-step cin0 / 16 (its readers passed the barrier that ended the previous chunk)
        __syncthreads();
        // ---- MFMAs: k-steps of 16 channels; per neighbour (di, dj) one fragment pair, then that neighbour's taps x 2 channel blocks x 3 products
#pragma unroll 1
        for (int S = 0; S < 2; ++S) {
            wfetch((cin0 >> 4) + S + 1);                                     // the next k-step's weights travel under these MFMAs
            const u32x4* wl = wbuf + hh * 64 + j;
            const u32x4* bl = patch + (2 * S + hh) * CP_PIX + wave * CP_W + j;
#pragma unroll
            for (int di = 0; di < 2; ++di)
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    __builtin_amdgcn_sched_barrier(0);                       // one neighbour's fragments at a time (register budget: 128 accumulators + 36 weight registers in flight)
                    const f16x8 bh = __builtin_bit_cast(f16x8, bl[di * CP_W + dj]);
                    const f16x8 bo = __builtin_bit_cast(f16x8, bl[CT_PART + di * CP_W + dj]);
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        if ((ky == 0) != (di == 1)) continue;                // di = 0: ky = 1, 2; di = 1: ky = 0
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            if ((kx == 0) != (dj == 1)) continue;
                            const int tap = ky * 3 + kx, ph = 2 * (ky == 1 ? 0 : 1) + (kx == 1 ? 0 : 1);
#pragma unroll
                            for (int cb = 0; cb < 2; ++cb) {
                                const f16x8 ah = __builtin_bit_cast(f16x8, wl[tap * 128 + cb * 32]);
                                const f16x8 al = __builtin_bit_cast(f16x8, wl[S_WPART + tap * 128 + cb * 32]);
                                const f16x8 as = ah * (_Float16)0.00048828125f;      // w_hi 2^-11: partner of the scaled x_lo'
                                // the two small cross terms first, then the leading term
                                acc[ph][cb] = mfma16(al, bh, acc[ph][cb]);
                                acc[ph][cb] = mfma16(as, bo, acc[ph][cb]);
                                acc[ph][cb] = mfma16(ah, bh, acc[ph][cb]);
                            }
                        }
                    }
                }
            __syncthreads();                                                 // weight buffer (and, after the chunk's last k-step, the patch) free
            if (S == 0) { wpark(); __syncthreads(); }
        }
    }

    // ---- epilogue: act(acc 2^-S + bias) at (2 ly + a, 2 lx + b).  D row (cout) = (reg & 3) + 8 (reg >> 2) + 4 hh, column (pixel) = j.
    const float unscale = reinterpret_cast<const float*>(p.wq)[1];          // 2^-S (header of the prepared weights)
    const int W2 = 2 * p.w;
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(ybase, 0, (int)((size_t)CT_C * p.yPlane * 4), 0x00020000);
    const int ly = oy0 + wave, lx = ox0 + j;
    const bool inside = ly < p.h && lx < p.w;
    const bool odd = (j & 1) != 0;
    const unsigned inmask = inside ? 0xffffffffu : 0u;                       // (lanes outside the image store nothing and report nothing)
    const bool hasBias = p.bias != nullptr;
    const float* const bias = hasBias ? p.bias : reinterpret_cast<const float*>(p.wq + 1);     // no bias: any 64 readable floats, then discarded (no branch per value)
    unsigned mag = 0u;
    isr_with_act(p.act, [&](auto A) {
        constexpr int ACT = decltype(A)::value;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int Y = 2 * ly + a;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) {
                __builtin_amdgcn_sched_barrier(0);
                float bv[16];                                                // the block's bias values first: one latency (L1 hits after the first row)
#pragma unroll
                for (int i = 0; i < 16; ++i) { const float b = bias[cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh]; bv[i] = hasBias ? b : 0.0f; }
                float v0[16], v1[16];                                        // phases (a, 0), (a, 1): output columns 2 lx, 2 lx + 1
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    v0[i] = isr_activate<ACT>(acc[2 * a][cb][i] * unscale + bv[i], p.slope);
                    v1[i] = isr_activate<ACT>(acc[2 * a + 1][cb][i] * unscale + bv[i], p.slope);
                    mag = isr_umax(mag, isr_umax(isr_mag(v0[i]), isr_mag(v1[i])) & inmask);
                }
                if (p.wide) {
                    // lanes (j, j ^ 1) and the channel pair (c, c + 1) of registers (2 t, 2 t + 1): the even lane keeps channel c and takes
                    // the odd lane's two pixels of it, the odd lane keeps c + 1 and takes the even lane's: columns 4 (j / 2) .. + 3 of one channel
                    const unsigned pixoff = inside ? (unsigned)(Y * W2 + 4 * (lx >> 1)) * 4u : BAD_OFFSET;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const int i0 = 2 * t, i1 = 2 * t + 1;
                        const float r0 = ct_swap1(odd ? v0[i0] : v0[i1]);
                        const float r1 = ct_swap1(odd ? v1[i0] : v1[i1]);
                        float4 q;
                        if (odd) { q.x = r0; q.y = r1; q.z = v0[i1]; q.w = v1[i1]; }
                        else { q.x = v0[i0]; q.y = v1[i0]; q.z = r0; q.w = r1; }
                        const int co = cb * 32 + ((odd ? i1 : i0) & 3) + 8 * (i0 >> 2) + 4 * hh;
                        // (soffset 0: sr_split_common.h)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, q), yrs,
                                                               (int)(inside ? pixoff + (unsigned)co * (unsigned)p.yPlane * 4u : BAD_OFFSET), 0, 0);
                    }
                } else {
                    const unsigned pixoff = inside ? (unsigned)(Y * W2 + 2 * lx) * 4u : BAD_OFFSET;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int co = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
                        const unsigned off = inside ? pixoff + (unsigned)co * (unsigned)p.yPlane * 4u : BAD_OFFSET;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v0[i]), yrs, (int)off, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v1[i]), yrs, (int)(inside ? off + 4u : BAD_OFFSET), 0, 0);
                    }
                }
            }
        }
    });
    isr_range_note(p.absmax, mag);
}

// ---- DATA GRADIENT ----------------------------------------------------------------------------------------------------------------
// gx[ci][i][j] = sum_{co, ky, kx} gz[co][2i - 1 + ky][2j - 1 + kx] w[ci][co][ky][kx] over the PHASE-MAJOR gradient G[4 co + 2 a + b][i][j] =
// gz[co][2i + a][2j + b] (isrConvTransposePhaseGradient): tap ky = 1 reads phase a = 0 at row i, ky = 2 reads a = 1 at row i, ky = 0 reads
// a = 1 at row i - 1; columns alike.  The forward kernel's dataflow with the halo row and column ABOVE and to the LEFT (index -1 is outside
// the image: zero), the roles of ci and co swapped in the weight image, and ONE accumulator set instead of four: the nine 64 x 64 products
// of a low-resolution pixel all land on the same output pixel.
//
// Structure: workgroup = 4 x 32 low-resolution pixels of one image x 64 output channels (ci), 4 waves, wave w owns row w: 2 channel blocks
// = 32 accumulator registers.  K runs phase-major: 8 chunks of (phase, 32 co) staged as LDS[hi | lo'][group of 8 co][5 x 33 patch pixels],
// two k-steps of 16 co each; a k-step of phase (a, b) multiplies that phase's 1, 2, 2 or 4 taps, each against its own neighbour (di, dj) in
// {0, -1}^2.  Weights [hi | lo][tap slot][lane half][64 ci] of one k-step pass through LDS, fetched into registers under the previous
// k-step's MFMAs.  Fixed summation order, no atomics on floats: the same bits on every run.  37.5 KB of LDS.
constexpr int ISR_VARIANT_CONVT_DGRAD = 38;                                  // convt3x3s2_dgrad_split_kernel (ops.VARIANT_NAMES)
constexpr int DG_WPART = 4 * 2 * 64;                                         // weights of one k-step, one part: [tap slot 0 .. 3][lane half][64 ci]
constexpr int DG_WUNITS = 2 * DG_WPART;
constexpr int DG_LDS_BYTES = (CT_PUNITS + DG_WUNITS) * 16;                   // 21 120 + 16 384 = 37 504

struct ConvTGradParams {
    const float* g; const u32x4* wq; float* gx;
    int h, w;                         // low-resolution size: G is [N][256][h][w], gx [N][64][h][w], both packed
    int tilesX, tilesY, tilesImage;
    unsigned* absmax;                 // range guard (may be NULL)
    unsigned* slotmax;                // per-wave maxima (may be NULL), as SplitConvParams::slotmax
};

// tap slot s of phase ph = 2 a + b: the tap 3 ky + kx it multiplies and the patch offset of the neighbour (di, dj) it reads
__device__ __forceinline__ void dg_slot(int ph, int s, int& tap, int& off)
{
    const int a = ph >> 1, b = ph & 1;
    const int sj = b ? (a ? (s & 1) : s) : 0;                                // 1: the column to the left (kx = 0)
    const int si = a ? (b ? (s >> 1) : s) : 0;                               // 1: the row above (ky = 0)
    const int ky = a ? (si ? 0 : 2) : 1, kx = b ? (sj ? 0 : 2) : 1;
    tap = 3 * ky + kx;
    off = -(si * CP_W + sj);
}

__global__ __launch_bounds__(S_THREADS, 2) void convt3x3s2_dgrad_split_kernel(const ConvTGradParams p)
{
    extern __shared__ u32x4 patch[];                                         // CT_PUNITS patch units, then the weight buffer
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, hh = lane >> 5;
    int bid;
    {   // an XCD (= an L2) gets a contiguous range of tiles
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = blockIdx.x & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (blockIdx.x >> 3);
    }
    const int n = bid / p.tilesImage, t = bid - n * p.tilesImage;
    const int tx = t % p.tilesX, ty = t / p.tilesX;
    const int oy0 = ty * CT_H, ox0 = tx * CT_W;                              // origin of the tile; the patch starts one row and column before it
    const int plane = p.h * p.w;

    const rsrc_t grs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.g + (size_t)n * 4 * CT_C * plane), 0, (int)((size_t)4 * CT_C * plane * 4), 0x00020000);
    const unsigned planeBytes = (unsigned)plane * 4u;
    u32x4* const wbuf = patch + CT_PUNITS;

    f32x16 acc[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cb][i] = 0.0f;

    // step = 4 ph + ks: k-step ks (16 co) of phase ph.  Its weights: up to 4 tap slots x 256 units [part][lane half][64 ci]; thread t moves unit
    // t of every slot: byte 16 t + 4096 (4 tap + ks) of the prepared image
    const rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4*>(p.wq + 1), 0, 9 * CT_KSTEPS * 4096, 0x00020000);
    u32x4* const wdst = wbuf + (tid >> 7) * DG_WPART + (tid & 127);
    u32x4 wreg[4];
    auto wfetch = [&](int step) {
        if (step >= 4 * CT_KSTEPS) return;
        const int ph = step >> 2, ks = step & 3, nt = (1 + (ph >> 1)) * (1 + (ph & 1));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int tap, off;
            dg_slot(ph, i, tap, off);
            if (i < nt) wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(wrs, tid * 16, (tap * CT_KSTEPS + ks) * 4096, 0);
        }
    };
    auto wpark = [&](int step) {
        const int ph = step >> 2, nt = (1 + (ph >> 1)) * (1 + (ph & 1));
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < nt) wdst[i * 128] = wreg[i];
    };
    wfetch(0);                                                               // in flight under the first staging

#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const int ph = q >> 1, co0 = (q & 1) * S_CHUNK, nt = (1 + (ph >> 1)) * (1 + (ph & 1));
        // ---- stage 32 co of phase ph, split into hi and lo' parts: unit = (group g of 8 co, patch pixel); rows oy0 - 1 .. oy0 + 3, columns
        //      ox0 - 1 .. ox0 + 31, zeros outside the image (the buffer load of the out-of-range offset returns 0)
        for (int u0 = tid; u0 < CT_PART; u0 += 3 * S_THREADS) {
            float v[3][8];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int u = u0 + k * S_THREADS;
                const int g = u / CP_PIX, pix = u - g * CP_PIX;
                const int r = pix / CP_W, c = pix - r * CP_W;
                const int iy = oy0 - 1 + r, ix = ox0 - 1 + c;
                const bool ok = u < CT_PART && iy >= 0 && ix >= 0 && iy < p.h && ix < p.w;
                const unsigned base = (unsigned)(4 * (co0 + g * 8) + ph) * planeBytes + (unsigned)(iy * p.w + ix) * 4u;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] = buf_load(grs, ok ? base + (unsigned)(4 * e) * planeBytes : BAD_OFFSET);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int u = u0 + k * S_THREADS;
                f16x8 qh, ql;
#pragma unroll
                for (int e = 0; e < 8; ++e) { _Float16 a, b; split16x(v[k][e], a, b); qh[e] = a; ql[e] = b; }
                if (u < CT_PART) { patch[u] = __builtin_bit_cast(u32x4, qh); patch[CT_PART + u] = __builtin_bit_cast(u32x4, ql); }
            }
        }
        wpark(2 * q);                                                        // (its readers passed the barrier that ended the previous chunk)
        __syncthreads();
#pragma unroll 1
        for (int S = 0; S < 2; ++S) {
            wfetch(2 * q + S + 1);                                           // the next k-step's weights travel under these MFMAs
            const u32x4* wl = wbuf + hh * 64 + j;
            const u32x4* bl = patch + (2 * S + hh) * CP_PIX + (wave + 1) * CP_W + (j + 1);
#pragma unroll 1
            for (int s = 0; s < nt; ++s) {
                int tap, off;
                dg_slot(ph, s, tap, off);
                const f16x8 bh = __builtin_bit_cast(f16x8, bl[off]);
                const f16x8 bo = __builtin_bit_cast(f16x8, bl[CT_PART + off]);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const f16x8 ah = __builtin_bit_cast(f16x8, wl[s * 128 + cb * 32]);
                    const f16x8 al = __builtin_bit_cast(f16x8, wl[DG_WPART + s * 128 + cb * 32]);
                    const f16x8 as = ah * (_Float16)0.00048828125f;          // w_hi 2^-11: partner of the scaled g_lo'
                    acc[cb] = mfma16(al, bh, acc[cb]);
                    acc[cb] = mfma16(as, bo, acc[cb]);
                    acc[cb] = mfma16(ah, bh, acc[cb]);
                }
            }
            __syncthreads();                                                 // weight buffer (and, after the chunk's last k-step, the patch) free
            if (S == 0) { wpark(2 * q + 1); __syncthreads(); }
        }
    }

    // ---- epilogue: acc 2^-S at (ly, lx).  D row (ci) = (reg & 3) + 8 (reg >> 2) + 4 hh, column (pixel) = j: a wave instruction writes two
    //      runs of 128 contiguous bytes
    const float unscale = reinterpret_cast<const float*>(p.wq)[1];
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.gx + (size_t)n * CT_C * plane, 0, (int)((size_t)CT_C * plane * 4), 0x00020000);
    const int ly = oy0 + wave, lx = ox0 + j;
    const bool inside = ly < p.h && lx < p.w;
    const unsigned pixoff = (unsigned)(ly * p.w + lx) * 4u;
    unsigned mag = 0u;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int ci = cb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
            const float v = acc[cb][i] * unscale;
            if (inside) mag = isr_umax(mag, isr_mag(v));
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, (int)(inside ? pixoff + (unsigned)ci * planeBytes : BAD_OFFSET), 0, 0);
        }
    if (p.slotmax) {
        unsigned m = mag;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = isr_umax(m, (unsigned)__shfl_xor((int)m, o, 64));
        if (lane == 0) atomicMax(p.slotmax + blockIdx.x * 4 + wave, m);
    }
    isr_range_note(p.absmax, mag);
}

bool convt_supported(int Cin, int Cout, int h, int w, long long xPlane, long long yPlane)
{
    if (Cin != CT_C || Cout != CT_C || h <= 0 || w <= 0 || h > 16384 || w > 16384) return false;
    if (xPlane < (long long)h * w || yPlane < 4LL * h * w) return false;
    // one image through 32-bit buffer offsets: input and output each below 2 GiB
    return xPlane * CT_C * 4 <= 0x7fffffffLL && yPlane * CT_C * 4 <= 0x7fffffffLL;
}

// the data gradient: N images, G [N][256][h][w] and gx [N][64][h][w] packed; one image of G through 32-bit buffer offsets
bool convt_dgrad_supported(int N, int C, int h, int w)
{
    if (C != CT_C || N <= 0 || h <= 0 || w <= 0 || h > 16384 || w > 16384) return false;
    if ((long long)h * w * 4 * CT_C * 4 > 0x7fffffffLL) return false;
    const long long grid = (long long)N * ((w + CT_W - 1) / CT_W) * ((h + CT_H - 1) / CT_H);
    return grid <= 0x3fffffffLL;
}

} // namespace

extern "C" {

int isrConvTranspose3x3S2DataGradSplitSupported(int N, int C, int h, int w)
{
    return convt_dgrad_supported(N, C, h, w) ? 1 : 0;
}

int isrConvTranspose3x3S2DataGradSplit(const float* G, const void* wq, float* gx, int N, int C, int h, int w, void* stream)
{
    unsigned* const rangeFlag = isr_take_range_flag();       // taken first: an error return must not leave it armed
    int slotCap = 0;
    unsigned* const slots = isr_take_max_slots(&slotCap);    // (likewise)
    if (!G || !wq || !gx) return -1;
    if (!convt_dgrad_supported(N, C, h, w)) return -3;
    ConvTGradParams p;
    p.g = G; p.wq = (const u32x4*)wq; p.gx = gx;
    p.h = h; p.w = w;
    p.tilesX = (w + CT_W - 1) / CT_W; p.tilesY = (h + CT_H - 1) / CT_H;
    p.tilesImage = p.tilesX * p.tilesY;
    p.absmax = rangeFlag;
    const long long grid = (long long)N * p.tilesImage;
    p.slotmax = nullptr;
    if (slots && 4 * grid <= slotCap) { p.slotmax = slots; isr_note_max_slot_words((int)(4 * grid)); }
    // algorithmic flops: 2 x 9 channel-mixing products of 64 x 64 per low-resolution pixel
    const double flops = 2.0 * 9 * CT_C * CT_C * (double)N * h * w;
    return isr_launch(ISR_VARIANT_CONVT_DGRAD, flops, convt3x3s2_dgrad_split_kernel, dim3((unsigned)grid), dim3(S_THREADS), DG_LDS_BYTES,
                      (hipStream_t)stream, p);
}

int isrConvTranspose3x3S2SplitSupported(int Cin, int Cout, int h, int w, long long xPlane, long long yPlane)
{
    return convt_supported(Cin, Cout, h, w, xPlane, yPlane) ? 1 : 0;
}

int isrConvTranspose3x3S2ForwardSplit(const float* x, const void* wq, const float* bias, float* y, int Cin, int h, int w, int Cout,
                                      int act, float slope, long long xPlane, long long yPlane, void* stream)
{
    unsigned* const rangeFlag = isr_take_range_flag();       // taken first: an error return must not leave it armed
    if (!x || !wq || !y || h <= 0 || w <= 0 || Cin <= 0 || Cout <= 0) return -1;
    if (act != ISR_ACT_NONE && act != ISR_ACT_RELU && act != ISR_ACT_LEAKY) return -1;
    if (!convt_supported(Cin, Cout, h, w, xPlane, yPlane)) return -3;
    ConvTParams p;
    p.x = x; p.wq = (const u32x4*)wq; p.bias = bias; p.y = y;
    p.h = h; p.w = w;
    p.xPlane = (int)xPlane; p.yPlane = (int)yPlane;
    p.tilesX = (w + CT_W - 1) / CT_W; p.tilesY = (h + CT_H - 1) / CT_H;
    p.act = act; p.slope = slope;
    p.wide = ((w & 1) == 0 && (yPlane & 3) == 0 && ((uintptr_t)y & 15) == 0) ? 1 : 0;
    p.absmax = rangeFlag;
    p.tilesImage = p.tilesX * p.tilesY; p.xImage = 0; p.yImage = 0;
    // algorithmic flops: 2 x 9 channel-mixing products of 64 x 64 per low-resolution pixel
    const double flops = 2.0 * 9 * CT_C * CT_C * (double)h * w;
    return isr_launch(ISR_VARIANT_CONVT_SPLIT, flops, convt3x3s2_split_kernel<false>, dim3((unsigned)(p.tilesX * p.tilesY)), dim3(S_THREADS), CT_LDS_BYTES,
                      (hipStream_t)stream, p);
}

int isrConvTranspose3x3S2ForwardSplitBatch(const float* x, const void* wq, const float* bias, float* y, int N, int h, int w,
                                           int act, float slope, void* stream)
{
    unsigned* const rangeFlag = isr_take_range_flag();       // taken first: an error return must not leave it armed
    if (!x || !wq || !y || N <= 0 || h <= 0 || w <= 0) return -1;
    if (act != ISR_ACT_NONE && act != ISR_ACT_RELU && act != ISR_ACT_LEAKY) return -1;
    const long long xPlane = (long long)h * w, yPlane = 4 * xPlane;
    if (!convt_supported(CT_C, CT_C, h, w, xPlane, yPlane)) return -3;
    ConvTParams p;
    p.x = x; p.wq = (const u32x4*)wq; p.bias = bias; p.y = y;
    p.h = h; p.w = w;
    p.xPlane = (int)xPlane; p.yPlane = (int)yPlane;
    p.tilesX = (w + CT_W - 1) / CT_W; p.tilesY = (h + CT_H - 1) / CT_H;
    p.act = act; p.slope = slope;
    p.wide = ((w & 1) == 0 && ((uintptr_t)y & 15) == 0) ? 1 : 0;           // (packed: every plane and image starts 4 h w floats after the last)
    p.absmax = rangeFlag;
    p.tilesImage = p.tilesX * p.tilesY; p.xImage = CT_C * xPlane; p.yImage = CT_C * yPlane;
    const long long grid = (long long)N * p.tilesImage;
    if (grid > 0x3fffffffLL) return -3;
    const double flops = 2.0 * 9 * CT_C * CT_C * (double)N * h * w;
    return isr_launch(ISR_VARIANT_CONVT_SPLIT, flops, convt3x3s2_split_kernel<true>, dim3((unsigned)grid), dim3(S_THREADS), CT_LDS_BYTES,
                      (hipStream_t)stream, p);
}

} // extern "C"
