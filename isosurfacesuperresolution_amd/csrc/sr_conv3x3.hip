// Fused 3x3 convolution (+bias +activation +residual, optional fused x2 bilinear upsample of the
// input) for MI355X / gfx950, fp32 in, fp32 accumulate, on the f32 MFMA pipe.
//
// Replaces the nn.Conv2d / nn.ReLU / residual add / nn.Upsample chain of the reference's
// EnhanceNet (SuperresolutionNetwork/models/enhancenet.py:92-125,136-144), which the reference
// runs as separate cuDNN / ATen calls.
//
// Formulation: implicit GEMM without im2col.  D[cout][pixel] = sum_k W[cout][k] * P[k][pixel],
// k = (tap, cin).  M = output channels (A operand = weights), N = 32 consecutive pixels of one
// image row (B operand = the input patch), so that each accumulator register is a 128-byte
// contiguous run of the NCHW output.  v_mfma_f32_32x32x2_f32 is an exact k-ordered fp32 fmaf chain
// (cdna_hip_programming.md section 3), which is what the 1e-4 parity bar needs.
//
// Workgroup = 4 waves = one 16x32 output tile for all output channels; wave w owns rows 4w..4w+3,
// i.e. MT x 4 accumulator tiles of 32x32.  The haloed 18x34 input patch is staged through LDS in
// chunks of 16 input channels (double buffered, register-staged so the x2 bilinear upsample can be
// fused into the loader); the 9 taps are 9 shifted ds_read_b32 views of the same patch (lanes
// 0-31 read 32 consecutive floats: conflict free).  Weights are read straight from L1/L2 in a
// [tap][cin][cout] layout (256 B per k-step and M tile; fp32 MFMA is so slow -- 64 cycles per
// instruction -- that this is ~4 B/clk/CU).
//
// This file: the exact fp32 forward kernels, the weight re-layout and their dispatcher.  The weight gradient is sr_wgrad.hip, the
// small-Cout kernel sr_conv_small.hip, the profiler's records sr_profile.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sr_conv_common.h"

namespace {

constexpr int TH = 16;            // tile rows
constexpr int TW = 32;            // tile cols (= MFMA N)
constexpr int PH = TH + 2;        // patch rows
constexpr int PW = TW + 2;        // patch cols
constexpr int CK = 16;            // input channels per LDS chunk
constexpr int PLANE = PH * PW;    // 612 floats per channel plane
constexpr int CHUNK = CK * PLANE; // 9792 floats per chunk

struct ConvParams {
    const float* x;
    const float* w;          // [9][cinPad][coutPad]
    const float* bias;
    const float* residual;
    float* y;
    int N, Cin, H, W, Cout;  // H, W: output size
    int Hin, Win;            // input size (H/2, W/2 when upsampling)
    int xPlane, yPlane, rPlane;          // channel strides of x / y / residual in floats (>= rows * cols)
    long long xImage, yImage, rImage;    // batch strides in floats
    int cinPad, coutPad;     // padded channel counts of the weight layout
    int co0;                 // first output channel handled by this launch (multiple of 64)
    int cgroups;             // conv3x3_fwd2_kernel: 32-channel groups covered by the grid (co0 + 32 g)
    int tilesX, tilesY;
    int act;
    float slope;
    ISR_DIAG_MEMBER(int, dbg, 0);                 // ablation bits for tools/bench_conv.py (0 in production)
    ISR_DIAG_MEMBER(unsigned long long*, stamps, nullptr);   // dbg & 8: per-workgroup s_memtime stamps (diagnostic builds only)
};

// Staging plan of one thread: element i (i < 45) of a chunk is patch position e = tid + 256*i,
// i.e. channel c = e / 612 of the chunk, patch row/col (r, col).  The byte offset of that element
// inside the chunk's 16 input planes does not depend on the chunk, so it is computed once per
// workgroup and kept in ONE register per element; out-of-image positions get PLAN_BAD (the
// buffer hardware then returns 0 = the conv's zero padding) and channels beyond Cin fall behind
// the descriptor's num_records.
// With the x2-upsampling loader (bilinear, align_corners=False: src = (dst+.5)/2-.5 clamped at 0)
// the word holds the offset of the top-left tap plus 4 flag bits: bits 0/1 = parity of the
// hi-res x/y (odd -> weight .25 on the +1 neighbour, even -> .75), bits 29/30 = "+1 neighbour
// exists" in x/y.  At the image borders (dst 0 and dst max) the neighbour flag is cleared, which
// makes both taps the same texel, so the border cases need no weight of their own.
constexpr unsigned PLAN_BAD = 0x80000000u;
constexpr unsigned PLAN_DX = 1u << 29, PLAN_DY = 1u << 30;

template <bool UPS, int CHUNK_ = CHUNK, int PLANE_ = PLANE>
__device__ __forceinline__ unsigned plan_element(const ConvParams& p, int e, int oy0, int ox0)
{
    const int c = e / PLANE_;
    const int rem = e - c * PLANE_;
    const int r = rem / PW;
    const int col = rem - r * PW;
    const int gy = oy0 + r - 1, gx = ox0 + col - 1;
    const bool ok = e < CHUNK_ && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
    if (!ok) return PLAN_BAD;
    if (!UPS) return (unsigned)((c * p.xPlane + gy * p.Win + gx) * 4);
    const int x0 = gx > 0 ? (gx - 1) >> 1 : 0, y0 = gy > 0 ? (gy - 1) >> 1 : 0;
    unsigned w = (unsigned)((c * p.xPlane + y0 * p.Win + x0) * 4) | (unsigned)(gx & 1) | ((unsigned)(gy & 1) << 1);
    if (gx > 0 && x0 < p.Win - 1) w |= PLAN_DX;
    if (gy > 0 && y0 < p.Hin - 1) w |= PLAN_DY;
    return w;
}

template <int MT, int R = 4>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[MT][R], float* smem, int n, int oy0, int ox0,
                                              int co0, int wave, int lane);

// ---- forward algorithm 0: one workgroup per CU, 64 output channels (diagnostics builds only: isrDebugSetForwardAlgo) ----
#ifdef ISR_DIAG
constexpr int STAGE_REGS = (CHUNK + NTHREADS - 1) / NTHREADS;   // 39
constexpr int STAGE_PER_TAP = (STAGE_REGS + 8) / 9;             // 5 patch elements per thread per tap
constexpr unsigned PLAN_OFF = 0x1FFFFFFCu;

// phase 1: issue the loads of one element (1 or 4 dwords)
template <bool UPS>
__device__ __forceinline__ void issue_element(rsrc_t rs, unsigned w, unsigned rowBytes, float (&raw)[UPS ? 4 : 1])
{
    if (!UPS) {
        raw[0] = buf_load(rs, w);
    } else {
        const unsigned off = (w & PLAN_BAD) ? PLAN_BAD : (w & PLAN_OFF);
        const unsigned dx = (w & PLAN_DX) ? 4u : 0u, dy = (w & PLAN_DY) ? rowBytes : 0u;
        raw[0] = buf_load(rs, off); raw[1] = buf_load(rs, off + dx);
        raw[2] = buf_load(rs, off + dy); raw[3] = buf_load(rs, off + dy + dx);
    }
}

// phase 2: the value that goes to LDS
template <bool UPS>
__device__ __forceinline__ float finish_element(unsigned w, const float (&raw)[UPS ? 4 : 1])
{
    if (!UPS) return raw[0];
    const float lx = (w & 1u) ? 0.25f : 0.75f, ly = (w & 2u) ? 0.25f : 0.75f;
    const float hx = 1.0f - lx, hy = 1.0f - ly;
    return hy * (hx * raw[0] + lx * raw[1]) + ly * (hx * raw[2] + lx * raw[3]);
}

template <int MT, bool UPS>
__global__ __launch_bounds__(NTHREADS, 1) void conv3x3_fwd_kernel(const ConvParams p)
{
    constexpr int CP = MT * 32;                 // padded couts handled by this launch
    constexpr int WCHUNK = 9 * CK * CP;         // weight floats per chunk
    constexpr int WSLICE4 = CK * CP / 4;        // float4 per tap slice (256 or 128)
    constexpr int NSTAGE = STAGE_PER_TAP * 9;   // 45 planned elements per thread (39 real)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* patch0 = smem;                       // [2][CHUNK]
    float* wlds0 = smem + 2 * CHUNK;            // [2][WCHUNK]
    float* dump = wlds0 + 2 * WCHUNK;           // [4*NTHREADS] write-only sink for masked-off staging lanes

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tilesPerImage = p.tilesX * p.tilesY;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int n = bid / tilesPerImage;
    const int t = bid - n * tilesPerImage;
    const int ty = t / p.tilesX, tx = t - ty * p.tilesX;
    const int oy0 = ty * TH, ox0 = tx * TW;

    unsigned long long st0 = 0, st1 = 0, st2 = 0;
    if (p.dbg & 8) st0 = __builtin_amdgcn_s_memtime();
    f32x16 acc[MT][4];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[m][r][i] = 0.0f;

    const int nchunks = p.cinPad / CK;
    const int planeIn = p.xPlane;
    const float* ximg = p.x + (size_t)n * p.xImage;
    const unsigned rowBytes = (unsigned)p.Win * 4u;
    // descriptor of the 16 input planes of `chunk` (channels >= Cin are out of range -> 0)
    auto chunk_rsrc = [&](int chunk) -> rsrc_t {
        const int left = p.Cin - chunk * CK;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg + (size_t)chunk * CK * planeIn), 0,
                                                 left > 0 ? left * planeIn * 4 : 0, 0x00020000);
    };

    unsigned plan[NSTAGE];
#pragma unroll
    for (int i = 0; i < NSTAGE; ++i) plan[i] = plan_element<UPS>(p, tid + i * NTHREADS, oy0, ox0);
    // weights: float4 `tid` of the [CK][CP] slice of (chunk, tap); rows are input channels
    const int wrow = min(tid, WSLICE4 - 1) / (CP / 4), wc4 = min(tid, WSLICE4 - 1) - wrow * (CP / 4);
    const float* wthread = p.w + (size_t)wrow * p.coutPad + p.co0 + wc4 * 4;
    auto weight_slice = [&](int chunk, int tap) -> float4 {
        return *reinterpret_cast<const float4*>(wthread + ((size_t)tap * p.cinPad + chunk * CK) * p.coutPad);
    };

    // prologue: chunk 0 in full, in batches of 13 loads in flight
    {
        const rsrc_t rs = chunk_rsrc(0);
        constexpr int NB = UPS ? 3 : 1;            // batches: 39 (or 3 x 13 x 4 taps) loads in flight
        constexpr int PB = STAGE_REGS / NB;
        static_assert(PB * NB == STAGE_REGS, "prologue batching");
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float raw[PB][UPS ? 4 : 1];
#pragma unroll
            for (int i = 0; i < PB; ++i) issue_element<UPS>(rs, plan[b * PB + i], rowBytes, raw[i]);
#pragma unroll
            for (int i = 0; i < PB; ++i) {
                const int e = tid + (b * PB + i) * NTHREADS;
                if (e < CHUNK) patch0[e] = finish_element<UPS>(plan[b * PB + i], raw[i]);
            }
        }
        float4 wv[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) wv[tap] = weight_slice(0, tap);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
            if (tid < WSLICE4) reinterpret_cast<float4*>(wlds0 + tap * CK * CP)[tid] = wv[tap];
    }
    __syncthreads();
    if (p.dbg & 8) st1 = __builtin_amdgcn_s_memtime();

    const int j = lane & 31;       // pixel column inside the tile / cout inside the M tile
    const int kh = lane >> 5;      // which of the 2 k values of the 32x32x2 MFMA this lane feeds

    auto load_ops = [&](float (&a)[MT], float (&b)[4], const float* w_, const float* p_, int kk) {
#pragma unroll
        for (int m = 0; m < MT; ++m) a[m] = w_[(2 * kk) * CP + m * 32];
#pragma unroll
        for (int r = 0; r < 4; ++r) b[r] = p_[(2 * kk) * PLANE + r * PW];
    };
    auto mfma_step = [&](const float (&a)[MT], const float (&b)[4]) {
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[m][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], b[r], acc[m][r], 0, 0, 0);
    };

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < nchunks && !(p.dbg & 1);
        const float* pb = patch0 + buf * CHUNK + kh * PLANE + (wave * 4) * PW + j;
        const float* wb = wlds0 + buf * WCHUNK + kh * CP + j;
        float* pnext = patch0 + (buf ^ 1) * CHUNK + tid;
        float* wnext = wlds0 + (buf ^ 1) * WCHUNK;
        const rsrc_t rsn = chunk_rsrc(chunk + 1);
        // Operand registers are double buffered by hand: the LDS reads of k-step kk+1 are issued
        // before the 8 MFMAs of k-step kk (512 cycles of cover); the taps are fully unrolled so
        // that every LDS address is base + immediate and the staging plan is indexed statically.
        //
        // Staging of the next chunk rides inside the MFMA regions, software pipelined over taps:
        // k-step i (< 6) of tap t issues the loads of element 6t+i (taps 0..6 cover the 39
        // elements) and, first, parks the element issued TWO taps earlier (128 MFMAs, ~3.4 us of
        // cover for an HBM miss) in the idle LDS buffer.  The weight slices go two per tap in
        // k-steps 6 and 7 of taps 0..4 with the same distance.  So every park happens inside the
        // tap loop, and the address / lerp VALU work sits in the shadow of the MFMAs.
        constexpr int EPT = 6;                      // elements issued per tap
        static_assert(EPT * 7 >= STAGE_REGS, "taps 0..6 must cover the chunk");
        float a0[MT], b0[4], a1[MT], b1[4];
        float raw[2][EPT][UPS ? 4 : 1];
        float4 wraw[2][2];
        load_ops(a0, b0, wb, pb, 0);
        // The plan words are loop invariant; without the opaque copy hipcc hoists the decoded
        // offsets / weights of all 39 elements out of the chunk loop (+150 live registers, spills).
        auto plan_word = [&](int q) -> unsigned {
            unsigned w = plan[q];
            asm volatile("" : "+v"(w));
            return w;
        };
        // No branch around any staging access (a branch makes hipcc's waitcnt pass fall back to
        // vmcnt(0) in front of every ds_write): lanes without an element write to the `dump` area.
        float* const plast = (tid < CHUNK - (STAGE_REGS - 1) * NTHREADS) ? pnext + (STAGE_REGS - 1) * NTHREADS : dump + tid;
        auto park = [&](int q, const float (&rw)[UPS ? 4 : 1]) {           // element q (static) -> LDS
            const float v = finish_element<UPS>(plan_word(q), rw);
            if (q < STAGE_REGS - 1) pnext[q * NTHREADS] = v;
            else if (q == STAGE_REGS - 1) *plast = v;
        };
        float4* const wdst = (WSLICE4 >= NTHREADS || tid < WSLICE4) ? reinterpret_cast<float4*>(wnext) + tid
                                                                    : reinterpret_cast<float4*>(dump) + tid;
        const int wstep = (WSLICE4 >= NTHREADS || tid < WSLICE4) ? CK * CP / 4 : 0;   // float4 per tap slice
        auto stage_work = [&](int tap, int kk) {  // called inside the MFMA region of k-step kk
            if (kk < EPT) {
                if (tap >= 2 && (tap - 2) * EPT + kk < STAGE_REGS) park((tap - 2) * EPT + kk, raw[tap & 1][kk]);
                const int q = tap * EPT + kk;
                if (tap <= 6 && q < STAGE_REGS) issue_element<UPS>(rsn, plan_word(q), rowBytes, raw[tap & 1][kk]);
            } else {
                const int h = kk - EPT;                                   // 0 or 1
                const int sp = (tap - 2) * 2 + h, si = tap * 2 + h;       // weight slices parked / issued
                if (tap >= 2 && sp < 9) wdst[sp * wstep] = wraw[tap & 1][h];
                if (si < 9) wraw[tap & 1][h] = weight_slice(chunk + 1, si);
            }
        };
        // `more` is hoisted out of the tap loop (two copies of the loop) for the same reason.
        auto run_taps = [&](auto MORE) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
            const int tn = tap + 1, dyn = tn / 3, dxn = tn - dyn * 3;
            const float* pt = pb + dy * PW + dx;
            const float* wt = wb + tap * CK * CP;
            const float* ptn = pb + dyn * PW + dxn;
            const float* wtn = wb + tn * CK * CP;
            // full scheduling fences between the LDS-read groups and the MFMA groups: left alone,
            // hipcc sinks each ds_read to just in front of its consumer (fewer live registers),
            // which re-exposes the LDS latency every k-step
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < CK / 2; kk += 2) {
                load_ops(a1, b1, wt, pt, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(a0, b0);
                if (decltype(MORE)::value) stage_work(tap, kk);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 2 < CK / 2) load_ops(a0, b0, wt, pt, kk + 2);
                else if (tap < 8) load_ops(a0, b0, wtn, ptn, 0);
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(a1, b1);
                if (decltype(MORE)::value) stage_work(tap, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        };
        if (more) run_taps(std::true_type{}); else run_taps(std::false_type{});
        __syncthreads();
    }

    if (p.dbg & 8) st2 = __builtin_amdgcn_s_memtime();
    conv_epilogue<MT>(p, acc, smem, n, oy0, ox0, p.co0, wave, lane);
    if ((p.dbg & 8) && tid == 0 && p.stamps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();
        unsigned long long* o = p.stamps + (size_t)blockIdx.x * 4;
        o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3;
    }
}

template <int MT>
constexpr size_t conv_fwd_lds_bytes() { return (size_t)(2 * CHUNK + 2 * 9 * CK * MT * 32 + 4 * NTHREADS) * sizeof(float); }
#endif  // ISR_DIAG

template <int MT, int R>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, f32x16 (&acc)[MT][R], float* smem, int n, int oy0, int ox0,
                                              int co0, int wave, int lane)
{
    const int j = lane & 31, kh = lane >> 5;
    // epilogue: D row (cout) = (reg&3) + 8*(reg>>2) + 4*(lane>>5), D col (pixel) = lane&31.
    // Output / residual go through buffer descriptors of image n: per-lane byte offset of the pixel
    // (BAD_OFFSET outside the image), per-register scalar offset of the channel plane; channels
    // >= Cout fall behind num_records and are dropped by the hardware.  No per-element branches.
    const int ox = ox0 + j;
    // y and the residual may have different channel strides: the per-lane offset is built from the pixel part
    // and the channel part separately for each of them
    const int outBytes = (int)((size_t)p.Cout * p.yPlane * 4);
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y + (size_t)n * p.yImage, 0, outBytes, 0x00020000);
    const rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.residual ? p.residual + (size_t)n * p.rImage : p.y), 0,
        p.residual ? (int)((size_t)p.Cout * p.rPlane * 4) : 0, 0x00020000);
    float bv[MT][16];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            bv[m][i] = p.bias[min(co0 + m * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh, p.Cout - 1)];
    const int planeBytes = p.yPlane * 4, rplaneBytes = p.rPlane * 4;
    isr_with_act(p.act, [&](auto A) {                                       // (one switch, not one per value: sr_act.h)
    constexpr int ACT = decltype(A)::value;
    if (((p.W | p.yPlane | p.rPlane) & 3) == 0) {
        // Wide path: each wave transposes one output row (64 couts x 32 pixels) through its own 8 KB
        // of the now idle LDS, so that a lane owns 4 consecutive pixels of one channel and the
        // global traffic is dwordx4 (4x fewer store instructions; the dword epilogue is store-issue
        // bound at ~7 B/clk/CU).  Bias/activation are applied on the way in, the residual on the way out.
        float* tr = smem + wave * (64 * 32);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int oy = oy0 + wave * R + r;
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float v = isr_activate<ACT>(acc[m][r][i] + bv[m][i], p.slope);
                    tr[(m * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh) * 32 + j] = v;
                }
            // same-wave hand-off: LDS operations of one wave complete in order
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
#pragma unroll
            for (int t = 0; t < MT * 4; ++t) {
                const int q = lane + 64 * t;                     // float4 index: cout = q/8, pixel group = q%8
                const int co = q >> 3, px = ox0 + (q & 7) * 4;
                const bool ok = oy < p.H && px < p.W && !(p.dbg & 2);
                const unsigned off = ok ? (unsigned)((oy * p.W + px) * 4) : BAD_OFFSET;
                const int soff = (co0 + co) * planeBytes;      // per lane -> goes into the vector offset
                float4 v = reinterpret_cast<const float4*>(tr)[q];
                const unsigned voffs = ok ? off + (unsigned)soff : BAD_OFFSET;
                if (p.residual) {
                    const unsigned roffs = ok ? off + (unsigned)((co0 + co) * rplaneBytes) : BAD_OFFSET;
                    const u32x4 rr = __builtin_amdgcn_raw_buffer_load_b128(rrs, (int)roffs, 0, 0);
                    const float4 rf = __builtin_bit_cast(float4, rr);
                    if (ACT == ISR_ACT_GATE) {
                        v.x = rf.x > 0.f ? v.x : 0.f; v.y = rf.y > 0.f ? v.y : 0.f;
                        v.z = rf.z > 0.f ? v.z : 0.f; v.w = rf.w > 0.f ? v.w : 0.f;
                    } else {
                        v.x += rf.x; v.y += rf.y; v.z += rf.z; v.w += rf.w;
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), yrs, (int)voffs, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(0xC07F);   // reads done before the next row overwrites the slab
        }
    } else {
    const unsigned khoff = (unsigned)(4 * kh) * (unsigned)planeBytes, rkhoff = (unsigned)(4 * kh) * (unsigned)rplaneBytes;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int oy = oy0 + wave * R + r;
        const bool pix_ok = ox < p.W && oy < p.H && !(p.dbg & 2);
        const unsigned pix = pix_ok ? (unsigned)((oy * p.W + ox) * 4) + khoff : BAD_OFFSET;
        const unsigned rpix = pix_ok ? (unsigned)((oy * p.W + ox) * 4) + rkhoff : BAD_OFFSET;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            float rv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int soff = (co0 + m * 32 + (i & 3) + 8 * (i >> 2)) * rplaneBytes;
                rv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrs, (int)rpix, soff, 0));
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int soff = (co0 + m * 32 + (i & 3) + 8 * (i >> 2)) * planeBytes;
                float v = isr_activate<ACT>(acc[m][r][i] + bv[m][i], p.slope);
                if (ACT == ISR_ACT_GATE) v = rv[i] > 0.f ? v : 0.f;
                else v += rv[i];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, (int)pix, soff, 0);
            }
        }
    }
    }
    });
}

// ---- forward, two workgroups per CU ------------------------------------------------------------
// Same implicit GEMM, re-budgeted so that TWO workgroups share a CU: one M tile (32 output channels)
// per workgroup and 8-channel chunks -> 66 KB of LDS and < 256 registers per wave.  The point is not
// the MFMA loop (it is the same 8 x 32x32x2 per k-step pair) but everything around it: with one
// workgroup per CU the prologue (first chunk from HBM), the per-chunk barriers and the epilogue
// (bias/act/residual/store) leave the matrix pipe idle ~15 % of a workgroup's life; with two, the
// other workgroup's waves issue MFMAs in those holes.  The price is that a tile's input patch is staged
// once per 32-channel group (both groups of a tile are adjacent workgroups on one XCD, so the second
// read is an L2 hit).
//
// x2-upsampling loader: the 18x34 hi-res patch is 9x17 "quads" of 2x2 pixels (rows 2a-1, 2a; columns
// 2b-1, 2b relative to the tile) that interpolate the SAME four source texels (bilinear,
// align_corners=False: odd pixels weigh the pair .75/.25, even pixels .25/.75; clamping the source
// coordinates to the image reproduces the border rule).  One thread does a whole quad: 4 loads and 16
// FMAs for 4 patch elements instead of 16 loads and 28 FMAs, two ds_write_b64.
//
// R = output rows per wave: 4 (tile 16x32) or 1 (tile 4x32).  The small tile is for small problems (the 32x32
// training crops, 128x128 previews): a 64->64 layer on 16 crops is 64 workgroups of the big tile for 512 slots,
// 256 of the small one; per workgroup it stages the same weights for a quarter of the MFMAs, which only pays when
// the GPU would otherwise idle.
constexpr int CK2 = 8;
constexpr int DUMP2 = 4 * NTHREADS;                                  // write-only sink behind each patch buffer
template <int R> struct Geo2 {
    static constexpr int TH_ = 4 * R;                                    // tile rows
    static constexpr int PH_ = TH_ + 2;                                  // patch rows
    static constexpr int PLANE_ = PH_ * PW;                              // floats per channel plane (612 / 204)
    static constexpr int CHUNK_ = CK2 * PLANE_;                          // 4896 / 1632 floats
    static constexpr int NEL_ = (CHUNK_ + NTHREADS - 1) / NTHREADS;      // 20 / 7 patch elements per thread and chunk
    static constexpr int QUADS_ = (PH_ / 2) * 17;                        // 2x2 quads per channel (x2 loader)
    static constexpr int NQ_ = QUADS_ * CK2;                             // 1224 / 408 quads per chunk
    static constexpr int NQT_ = (NQ_ + NTHREADS - 1) / NTHREADS;         // 5 / 2 per thread
    static constexpr int PSTRIDE_ = CHUNK_ + DUMP2;                      // patch buffer + its sink
};
constexpr int WCH2 = 9 * CK2 * 32;                                   // 2304 weight floats per chunk
constexpr int NW42 = WCH2 / 4;                                       // 576 float4
constexpr int NWI2 = (NW42 + NTHREADS - 1) / NTHREADS;               // 3 per thread
constexpr int KSTEPS2 = CK2 / 2;                                     // 4 k-steps per tap
constexpr int NSLOTS2 = 9 * KSTEPS2;                                 // 36 k-steps per chunk = staging slots
// LDS: [2][WCH2] weights, then 2 x ([CHUNK_] patch, [DUMP2] sink): a masked-off staging lane keeps its
// offset and lands in the sink of whichever buffer is being filled.  (The epilogue transposes through the first
// 4 x 8 KB of it.)
template <int R>
constexpr size_t conv_fwd2_lds_bytes() { return (size_t)(2 * WCH2 + 2 * Geo2<R>::PSTRIDE_) * sizeof(float); }
static_assert(conv_fwd2_lds_bytes<1>() >= 4 * 64 * 32 * sizeof(float), "epilogue slab");

constexpr unsigned Q_DX = 1u, Q_DY = 2u, Q_VX0 = 4u, Q_VX1 = 8u, Q_VY0 = 16u, Q_VY1 = 32u;   // aux bits; LDS float offset << 8

template <bool UPS, int R>
__global__ __launch_bounds__(NTHREADS, 2) void conv3x3_fwd2_kernel(const ConvParams p)
{
    typedef Geo2<R> G;
    constexpr int PLANE_ = G::PLANE_, CHUNK2 = G::CHUNK_, NEL2 = G::NEL_, QUADS2 = G::QUADS_, NQ2 = G::NQ_, NQT2 = G::NQT_, PSTRIDE2 = G::PSTRIDE_;
    constexpr int NEL = UPS ? NQT2 : NEL2;      // patch staging items per thread and chunk
    constexpr int NLD = UPS ? 4 : 1;            // loads per item
    constexpr int NITEMS = NEL + NWI2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wlds0 = smem;                        // [2][9][CK2][32]
    float* patch0 = smem + 2 * WCH2;            // 2 x (patch, sink)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int tilesPerImage = p.tilesX * p.tilesY;
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int grp = lid % p.cgroups;            // the channel groups of one tile are neighbours on one XCD
    const int bid = lid / p.cgroups;
    const int n = bid / tilesPerImage;
    const int t = bid - n * tilesPerImage;
    const int ty = t / p.tilesX, tx = t - ty * p.tilesX;
    const int oy0 = ty * G::TH_, ox0 = tx * TW;
    const int co0 = p.co0 + grp * 32;

    unsigned long long st0 = 0, st1 = 0, st2 = 0;
    if (p.dbg & 8) st0 = __builtin_amdgcn_s_memtime();
    f32x16 acc[1][R];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[0][r][i] = 0.0f;

    const int nchunks = (p.Cin + CK2 - 1) / CK2;     // weight rows >= Cin are zero, input planes >= Cin read as 0
    const int planeIn = p.xPlane;
    const float* ximg = p.x + (size_t)n * p.xImage;
    const unsigned rowBytes = (unsigned)p.Win * 4u;
    auto chunk_rsrc = [&](int chunk) -> rsrc_t {
        const int left = p.Cin - chunk * CK2;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ximg + (size_t)chunk * CK2 * planeIn), 0,
                                                 left > 0 ? left * planeIn * 4 : 0, 0x00020000);
    };

    // Staging plan, one or two words per item, chunk invariant.
    //  plain: plan = byte offset of the element in the chunk's planes (PLAN_BAD outside the image);
    //         item i is patch element tid + 256 i and goes to that float of the patch buffer.
    //  UPS:   plan = byte offset of the quad's top-left source texel (clamped into the image),
    //         aux  = Q_* flags | (float offset of the quad's first element in the patch buffer) << 8.
    unsigned plan[NEL], aux[UPS ? NEL : 1];
    if (UPS) {
        const int m0 = (oy0 >> 1) - 1, q0 = (ox0 >> 1) - 1;
#pragma unroll
        for (int i = 0; i < NEL; ++i) {
            const int qi = tid + i * NTHREADS;
            const int c = qi / QUADS2, rem = qi - c * QUADS2;
            const int a = rem / 17, b = rem - a * 17;
            const int m = m0 + a, q = q0 + b;                          // source row / column of the top-left texel
            const int r0 = min(max(m, 0), p.Hin - 1), r1 = min(max(m + 1, 0), p.Hin - 1);
            const int c0 = min(max(q, 0), p.Win - 1), c1 = min(max(q + 1, 0), p.Win - 1);
            const int gy = oy0 - 1 + 2 * a, gx = ox0 - 1 + 2 * b;      // hi-res coordinates of the quad's first pixel
            unsigned f = 0;
            if (c1 != c0) f |= Q_DX;
            if (r1 != r0) f |= Q_DY;
            if ((unsigned)gx < (unsigned)p.W) f |= Q_VX0;
            if ((unsigned)(gx + 1) < (unsigned)p.W) f |= Q_VX1;
            if ((unsigned)gy < (unsigned)p.H) f |= Q_VY0;
            if ((unsigned)(gy + 1) < (unsigned)p.H) f |= Q_VY1;
            const bool exists = qi < NQ2;
            plan[i] = exists ? (unsigned)((c * p.xPlane + r0 * p.Win + c0) * 4) : PLAN_BAD;
            aux[i] = f | (unsigned)(exists ? c * PLANE_ + (2 * a) * PW + 2 * b : CHUNK2 + 2 * tid) << 8;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NEL; ++i) plan[i] = plan_element<false, CHUNK2, PLANE_>(p, tid + i * NTHREADS, oy0, ox0);
    }
    // weights: float4 f = tid + 256 i of the chunk's [9][CK2][32] block; f = tap*64 + k*8 + c4
    unsigned woff[NWI2];
#pragma unroll
    for (int i = 0; i < NWI2; ++i) {
        const int f = min(tid + i * NTHREADS, NW42 - 1);
        const int tap = f >> 6, k = (f >> 3) & 7, c4 = f & 7;
        woff[i] = (unsigned)((tap * p.cinPad + k) * p.coutPad + co0 + c4 * 4);
    }
    const float* wchunk = p.w;
    const size_t wchunkStep = (size_t)CK2 * p.coutPad;
    auto weight_item = [&](const float* base, int i) -> float4 { return *reinterpret_cast<const float4*>(base + woff[i]); };

    auto issue_patch = [&](rsrc_t rs, unsigned w, unsigned a, float (&raw)[NLD]) {
        if (UPS) {
            const unsigned dx = (a & Q_DX) ? 4u : 0u, dy = (a & Q_DY) ? rowBytes : 0u;
            raw[0] = buf_load(rs, w); raw[UPS ? 1 : 0] = buf_load(rs, w + dx);
            raw[UPS ? 2 : 0] = buf_load(rs, w + dy); raw[UPS ? 3 : 0] = buf_load(rs, w + dy + dx);
        } else {
            raw[0] = buf_load(rs, w);
        }
    };
    // UPS: the four pixels of a quad from its four texels, zeroed outside the image (the conv's padding)
    auto park_quad = [&](float* pbuf, unsigned a, const float (&raw)[NLD]) {
        const float t00 = raw[0], t01 = raw[UPS ? 1 : 0], t10 = raw[UPS ? 2 : 0], t11 = raw[UPS ? 3 : 0];
        const float top0 = __builtin_fmaf(0.25f, t01, 0.75f * t00), top1 = __builtin_fmaf(0.75f, t01, 0.25f * t00);
        const float bot0 = __builtin_fmaf(0.25f, t11, 0.75f * t10), bot1 = __builtin_fmaf(0.75f, t11, 0.25f * t10);
        float v00 = __builtin_fmaf(0.25f, bot0, 0.75f * top0), v01 = __builtin_fmaf(0.25f, bot1, 0.75f * top1);
        float v10 = __builtin_fmaf(0.75f, bot0, 0.25f * top0), v11 = __builtin_fmaf(0.75f, bot1, 0.25f * top1);
        const int ia = (int)a;
        const unsigned mx0 = (unsigned)__builtin_amdgcn_sbfe(ia, 2, 1), mx1 = (unsigned)__builtin_amdgcn_sbfe(ia, 3, 1);
        const unsigned my0 = (unsigned)__builtin_amdgcn_sbfe(ia, 4, 1), my1 = (unsigned)__builtin_amdgcn_sbfe(ia, 5, 1);
        auto masked = [](float v, unsigned m) { return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & m); };
        v00 = masked(v00, mx0 & my0); v01 = masked(v01, mx1 & my0);
        v10 = masked(v10, mx0 & my1); v11 = masked(v11, mx1 & my1);
        float* d = pbuf + (a >> 8);
        *reinterpret_cast<float2*>(d) = make_float2(v00, v01);
        *reinterpret_cast<float2*>(d + PW) = make_float2(v10, v11);
    };

    // prologue: chunk 0 in full
    {
        const rsrc_t rs = chunk_rsrc(0);
        float4 wv[NWI2];
#pragma unroll
        for (int i = 0; i < NWI2; ++i) wv[i] = weight_item(wchunk, i);
        float raw[NEL][NLD];
#pragma unroll
        for (int i = 0; i < NEL; ++i) issue_patch(rs, plan[i], UPS ? aux[UPS ? i : 0] : 0u, raw[i]);
#pragma unroll
        for (int i = 0; i < NEL; ++i) {
            if (UPS) park_quad(patch0, aux[UPS ? i : 0], raw[i]);
            else if (tid + i * NTHREADS < CHUNK2) patch0[tid + i * NTHREADS] = raw[i][0];
        }
#pragma unroll
        for (int i = 0; i < NWI2; ++i)
            if (tid + i * NTHREADS < NW42) reinterpret_cast<float4*>(wlds0)[tid + i * NTHREADS] = wv[i];
    }
    __syncthreads();
    if (p.dbg & 8) st1 = __builtin_amdgcn_s_memtime();

    const int j = lane & 31;
    const int kh = lane >> 5;
    auto load_ops = [&](float& a, float (&b)[R], const float* w_, const float* p_, int kk) {
        a = w_[(2 * kk) * 32];
#pragma unroll
        for (int r = 0; r < R; ++r) b[r] = p_[(2 * kk) * PLANE_ + r * PW];
    };
    auto mfma_step = [&](float a, const float (&b)[R]) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[0][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[r], acc[0][r], 0, 0, 0);
    };

    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < nchunks && !(p.dbg & 1);
        const float* pb = patch0 + buf * PSTRIDE2 + kh * PLANE_ + (wave * R) * PW + j;
        const float* wb = wlds0 + buf * WCH2 + kh * 32 + j;
        float* const pfill = patch0 + (buf ^ 1) * PSTRIDE2;          // buffer being filled (+ its sink)
        float* const pnext = pfill + tid;
        float4* const wnext = reinterpret_cast<float4*>(wlds0 + (buf ^ 1) * WCH2) + tid;
        const rsrc_t rsn = chunk_rsrc(chunk + 1);
        wchunk += wchunkStep;                       // now the next chunk's weight rows (only read when `more`)
        float a0, b0[R], a1, b1[R];
        float raw[NEL][NLD];
        float4 wraw[NWI2];
        load_ops(a0, b0, wb, pb, 0);
        auto opaque = [&](unsigned w) -> unsigned {   // keeps hipcc from hoisting the decode of every item out of the loop
            asm volatile("" : "+v"(w));
            return w;
        };
        float* const plast = (tid < CHUNK2 - (NEL2 - 1) * NTHREADS) ? pnext + (NEL2 - 1) * NTHREADS : pfill + CHUNK2 + tid;
        float4* const wlast = (tid < NW42 - (NWI2 - 1) * NTHREADS) ? wnext + (NWI2 - 1) * NTHREADS
                                                                   : reinterpret_cast<float4*>(pfill + CHUNK2) + tid;
        // Staging of the next chunk rides in the MFMA slots (slot s = k-step s of the chunk, 36 per
        // chunk), all loads early and all LDS writes late so that every load has >= 20 k-steps
        // (>= 5000 cycles) to come back.  No branches around the memory operations: a branch makes
        // hipcc's waitcnt pass fall back to vmcnt(0).
        //   plain: items issued two per slot in slots 0..11, parked two per slot in slots 24..35
        //   UPS:   quad i issued in slot 2i, weights in slots 10..12; quad i parked in slot 20+3i, weights 33..35
        auto park_item = [&](int q) {
            if (q < NEL) {
                if (UPS) park_quad(pfill, opaque(aux[UPS ? q : 0]), raw[q]);
                else if (q < NEL - 1) pnext[q * NTHREADS] = raw[q][0];
                else *plast = raw[q][0];
            } else {
                const int i = q - NEL;
                if (i < NWI2 - 1) wnext[i * NTHREADS] = wraw[i]; else *wlast = wraw[i];
            }
        };
        auto issue_item = [&](int q) {
            if (q < NEL) issue_patch(rsn, opaque(plan[q]), UPS ? opaque(aux[UPS ? q : 0]) : 0u, raw[q]);
            else wraw[q - NEL] = weight_item(wchunk, q - NEL);
        };
        auto slot = [&](int s) {
            if (UPS) {
                if (s >= 20 && s < 20 + 3 * NEL && (s - 20) % 3 == 0) park_item((s - 20) / 3);
                if (s >= NSLOTS2 - NWI2) park_item(NEL + s - (NSLOTS2 - NWI2));
                if (s < 2 * NEL && s % 2 == 0) issue_item(s / 2);
                if (s >= 2 * NEL && s < 2 * NEL + NWI2) issue_item(NEL + s - 2 * NEL);
            } else {
                constexpr int PARK0 = NSLOTS2 - (NITEMS + 1) / 2;     // 24
                static_assert(UPS || PARK0 >= (NITEMS + 1) / 2, "issue phase must end before the park phase starts");
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int qp = (s - PARK0) * 2 + h;
                    if (s >= PARK0 && qp < NITEMS) park_item(qp);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int q = s * 2 + h;
                    if (q < NITEMS) issue_item(q);
                }
            }
        };
        static_assert(20 + 3 * (NQT2 - 1) < NSLOTS2 - NWI2 && 2 * NQT2 + NWI2 <= 20, "UPS staging schedule");
        static_assert(CHUNK2 + 2 * NTHREADS + PW + 2 <= PSTRIDE2, "the quad sink must stay inside the buffer's sink");
        auto run_taps = [&](auto MORE) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
            const int tn = tap + 1, dyn = tn / 3, dxn = tn - dyn * 3;
            const float* pt = pb + dy * PW + dx;
            const float* wt = wb + tap * CK2 * 32;
            const float* ptn = pb + dyn * PW + dxn;
            const float* wtn = wb + tn * CK2 * 32;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < KSTEPS2; kk += 2) {
                load_ops(a1, b1, wt, pt, kk + 1);
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(a0, b0);
                if (decltype(MORE)::value) slot(tap * KSTEPS2 + kk);
                __builtin_amdgcn_sched_barrier(0);
                if (kk + 2 < KSTEPS2) load_ops(a0, b0, wt, pt, kk + 2);
                else if (tap < 8) load_ops(a0, b0, wtn, ptn, 0);
                __builtin_amdgcn_sched_barrier(0);
                mfma_step(a1, b1);
                if (decltype(MORE)::value) slot(tap * KSTEPS2 + kk + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        };
        if (more) run_taps(std::true_type{}); else run_taps(std::false_type{});
        __syncthreads();
    }
    if (p.dbg & 8) st2 = __builtin_amdgcn_s_memtime();
    conv_epilogue<1, R>(p, acc, smem, n, oy0, ox0, co0, wave, lane);
    if ((p.dbg & 8) && tid == 0 && p.stamps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();
        unsigned long long* o = p.stamps + (size_t)blockIdx.x * 4;
        o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3;
    }
}

// ---- forward for small problems: one output row per workgroup, K split over the waves -------------
// A batch of 32x32 training crops is 256 workgroups of the 4x32 tiling (16 crops; 32 for the two crops per GPU of
// BASELINE config #3): at most one wave per SIMD, each running its 288 dependent k-steps alone -- 13 us of workgroup
// life however few pixels there are.  Here a workgroup is ONE output row of 32 pixels x 32 output channels and its
// four waves split the input channels; partial sums meet in LDS.  Four times the workgroups with a quarter of the
// serial chain each.  Operands come straight from global memory / L2 (one dword per lane and MFMA operand, both
// coalesced: weights [tap][ci][co] along co, pixels along x) through buffer descriptors whose out-of-range reads
// return the zero padding; no staging, no barriers in the loop.  The loads bound it: a dword-per-lane buffer load
// occupies the texture path for 16 cycles per wave (stamps: 9200 cycles for the 4 x 144 loads of a CU's workgroup,
// the 72 MFMAs of a wave are 4600).  Tried and dropped: channel / tap offsets as the instruction's scalar offset
// (45 % slower), one dwordx3 load per patch row (dword-aligned multi-dword buffer loads return the first dword in
// every component on this part), a second accumulator (no change: the chain is not what the wave waits for).
constexpr int ROW_VARIANT = 12;

__global__ __launch_bounds__(NTHREADS) void conv3x3_rowsplit_kernel(const ConvParams p)
{
    constexpr int KSB = 8;      // k-steps per block of up-front operand loads (144 registers; with 4 and more waves per
                                // SIMD the kernel is L1/TA bound and loses to the LDS-staged tiling from ~200 tiles on)
    __shared__ float part[4][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, kh = lane >> 5;
    int bid = blockIdx.x;
    const int cg = bid % p.cgroups; bid /= p.cgroups;
    const int tx = bid % p.tilesX; bid /= p.tilesX;
    const int oy = bid % p.H, n = bid / p.H;
    const int ox0 = tx * 32, co0 = cg * 32;

    const int chPerWave = p.cinPad >> 2;                     // cinPad is a multiple of 16
    const int c0 = wave * chPerWave;
    const rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.x + (size_t)n * p.xImage), 0,
                                                         (int)((size_t)p.Cin * p.xPlane * 4), 0x00020000);
    const rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, (int)((size_t)9 * p.cinPad * p.coutPad * 4), 0x00020000);
    // per-lane pixel offsets of the 9 taps inside a channel plane (BAD_OFFSET = zero padding)
    unsigned xoff[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = oy + t / 3 - 1, ix = ox0 + j + t % 3 - 1;
        xoff[t] = ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) ? (unsigned)(iy * p.W + ix) * 4u : BAD_OFFSET;
    }
    const unsigned planeBytes = (unsigned)p.xPlane * 4u;
    const unsigned wTap = (unsigned)(p.cinPad * p.coutPad) * 4u, wRow = (unsigned)p.coutPad * 4u;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

    // a block of KS k-steps (2 channels each): ALL operand loads are issued before the first MFMA, so the wave pays
    // one L2 round trip per block instead of one per k-step (there is no other wave on the SIMD to hide it)
    auto block = [&](auto ks_tag, int c) {
        constexpr int KS = decltype(ks_tag)::value;
        float a[KS][9], b[KS][9];
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            const unsigned ci = (unsigned)(c + 2 * k + kh);
            const unsigned cx = ci * planeBytes;
            const unsigned cw = ci * wRow + (unsigned)(co0 + j) * 4u;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                a[k][t] = buf_load(wrs, cw + (unsigned)t * wTap);
                b[k][t] = buf_load(xrs, xoff[t] == BAD_OFFSET ? BAD_OFFSET : cx + xoff[t]);
            }
        }
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k][t], b[k][t], acc, 0, 0, 0);
    };
    unsigned long long st0 = 0, st1 = 0, st2 = 0;
    if (p.dbg & 8) st0 = __builtin_amdgcn_s_memtime();
    int c = c0, rem = chPerWave >> 1;
    for (; rem >= KSB; rem -= KSB, c += 2 * KSB) block(std::integral_constant<int, KSB>{}, c);
    for (; rem >= 2; rem -= 2, c += 4) block(std::integral_constant<int, 2>{}, c);
    if (p.dbg & 8) { st1 = __builtin_amdgcn_s_memtime(); }
#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][i][lane] = acc[i];
    __syncthreads();
    // wave w finishes accumulator registers 4w .. 4w+3: D row (cout) = (reg & 3) + 8 * (reg >> 2) + 4 * kh, col (pixel) = j
    const int ox = ox0 + j;
    const rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(p.y + (size_t)n * p.yImage, 0, (int)((size_t)p.Cout * p.yPlane * 4), 0x00020000);
    const rsrc_t rrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.residual ? p.residual + (size_t)n * p.rImage : p.y), 0,
                                                         p.residual ? (int)((size_t)p.Cout * p.rPlane * 4) : 0, 0x00020000);
    const unsigned pix = ox < p.W ? (unsigned)(oy * p.W + ox) * 4u : BAD_OFFSET;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int reg = wave * 4 + q;
        const int co = co0 + (reg & 3) + 8 * (reg >> 2) + 4 * kh;
        float v = (part[0][reg][lane] + part[1][reg][lane]) + (part[2][reg][lane] + part[3][reg][lane]);
        v += p.bias[min(co, p.Cout - 1)];
        if (p.act == ISR_ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (p.act == ISR_ACT_LEAKY) v = v > 0.f ? v : v * p.slope;
        const bool ok = pix != BAD_OFFSET && co < p.Cout;
        if (p.residual) {
            const float r = buf_load(rrs, ok ? pix + (unsigned)co * (unsigned)p.rPlane * 4u : BAD_OFFSET);
            if (p.act == ISR_ACT_GATE) v = r > 0.f ? v : 0.f; else v += r;
        }
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), yrs, ok ? (int)(pix + (unsigned)co * (unsigned)p.yPlane * 4u) : (int)BAD_OFFSET, 0, 0);
    }
    if ((p.dbg & 8) && tid == 0 && p.stamps) {
        st2 = __builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st3 = __builtin_amdgcn_s_memtime();
        unsigned long long* o = p.stamps + (size_t)blockIdx.x * 4;
        o[0] = st0; o[1] = st1; o[2] = st2; o[3] = st3;
    }
}

// ---- weight re-layout ------------------------------------------------------------------------
__global__ void prepare_weights_kernel(const float* __restrict__ w, float* __restrict__ wp,
                                       int Cout, int Cin, int cinPad, int coutPad, int transpose_flip)
{
    // wp[tap][ci'][co'] ; forward: ci'=ci, co'=co ; data-grad: ci'=co, co'=ci, taps flipped
    const int total = 9 * cinPad * coutPad;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int co_ = e % coutPad;
        const int ci_ = (e / coutPad) % cinPad;
        const int tap = e / (coutPad * cinPad);
        const int ky = tap / 3, kx = tap % 3;
        float v = 0.0f;
        if (!transpose_flip) {
            if (ci_ < Cin && co_ < Cout) v = w[((co_ * Cin + ci_) * 3 + ky) * 3 + kx];
        } else {
            if (ci_ < Cout && co_ < Cin) v = w[((ci_ * Cin + co_) * 3 + (2 - ky)) * 3 + (2 - kx)];
        }
        wp[e] = v;
    }
}

}  // namespace

// The plan's switches: real variables behind isrDebugSet* in the diagnostics build, compile-time constants in the product.
#ifdef ISR_DIAG
#define ISR_PLAN_SWITCH static
int g_conv_dbg = 0;           // (shared with sr_wgrad.hip: sr_conv_common.h)
static unsigned long long* g_conv_stamps = nullptr;
static int g_conv_algo = 1;   // 0: one workgroup per CU (64 channels), 1: two per CU (32 channels each) -- the product's only form
#else
#define ISR_PLAN_SWITCH static constexpr
#endif
ISR_PLAN_SWITCH int g_conv_tile = 0;   // 0: automatic, 1: always 4x32 tiles, 2: always 16x32 tiles, 3: one row per workgroup (tools / tests)
ISR_PLAN_SWITCH long long g_row_threshold = 160;   // automatic: rows when the 4x32 tiling has at most this many workgroups
                                          // (HIP-graph chain of 64 -> 64 layers on N crops of 32x32, rows vs 4x32 tiles:
                                          //  N=2 7.5 vs 15.1 us, N=4 8.4 vs 15.2, N=8 12.1 vs 15.1, N=12 16.1 vs 16.0, N=16 19.5 vs 16.1)
#undef ISR_PLAN_SWITCH

extern "C" {

#ifdef ISR_DIAG
void isrDebugSetAblation(int bits) { g_conv_dbg = bits; }
void isrDebugSetForwardAlgo(int a) { g_conv_algo = a; }
void isrDebugSetForwardTile(int t) { g_conv_tile = t; }   // not part of the public header
void isrDebugSetRowThreshold(long long n) { g_row_threshold = n; }
void isrDebugSetStampBuffer(void* p) { g_conv_stamps = (unsigned long long*)p; }
#endif

int isrConvCinPad(int Cin) { return ((Cin + CK - 1) / CK) * CK; }
int isrConvCoutPad(int Cout) { return ((Cout + 31) / 32) * 32; }

int isrConvPrepareWeights(const float* w, float* wprep, int Cout, int Cin, int transpose_flip, void* stream)
{
    if (!w || !wprep || Cout <= 0 || Cin <= 0) return -1;
    const int cinPad = transpose_flip ? isrConvCinPad(Cout) : isrConvCinPad(Cin);
    const int coutPad = transpose_flip ? isrConvCoutPad(Cin) : isrConvCoutPad(Cout);
    const int total = 9 * cinPad * coutPad;
    const int blocks = (total + 255) / 256;
    hipLaunchKernelGGL(prepare_weights_kernel, dim3(blocks > 1024 ? 1024 : blocks), dim3(256), 0, (hipStream_t)stream,
                       w, wprep, Cout, Cin, cinPad, coutPad, transpose_flip);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int isrConv3x3Forward(const float* x, const float* wprep, const float* bias, const float* residual, float* y,
                      int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x, void* stream)
{
    if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return -1;
    const long long xp = upsample2x ? (long long)(H / 2) * (W / 2) : (long long)H * W, yp = (long long)H * W;
    return isrConv3x3ForwardStrided(x, wprep, bias, residual, y, N, Cin, H, W, Cout, act, slope, upsample2x,
                                    xp, xp * Cin, yp, yp * Cout, yp, yp * Cout, stream);
}

int isrConv3x3ForwardStrided(const float* x, const float* wprep, const float* bias, const float* residual, float* y,
                             int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x,
                             long long xPlane, long long xImage, long long yPlane, long long yImage,
                             long long rPlane, long long rImage, void* stream)
{
    if (!x || !wprep || !y || N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return -1;
    if (upsample2x && ((H & 1) || (W & 1))) return -1;
    if (act < ISR_ACT_NONE || act > ISR_ACT_GATE) return -1;
    if (act == ISR_ACT_GATE && !residual) return -1;
    {
        const long long rowsIn = (long long)(upsample2x ? H / 2 : H) * (upsample2x ? W / 2 : W);
        if (xPlane < rowsIn || yPlane < (long long)H * W || (residual && rPlane < (long long)H * W)) return -1;
        // buffer descriptors address one image with 32-bit byte offsets
        if (xPlane * Cin * 4 > 0x7fffffffLL || yPlane * Cout * 4 > 0x7fffffffLL || (residual && rPlane * Cout * 4 > 0x7fffffffLL)) return -1;
    }
    ConvParams p;
    p.x = x; p.w = wprep; p.bias = bias; p.residual = residual; p.y = y;
    p.N = N; p.Cin = Cin; p.H = H; p.W = W; p.Cout = Cout;
    p.Hin = upsample2x ? H / 2 : H; p.Win = upsample2x ? W / 2 : W;
    p.xPlane = (int)xPlane; p.yPlane = (int)yPlane; p.rPlane = (int)(residual ? rPlane : yPlane);
    p.xImage = xImage; p.yImage = yImage; p.rImage = rImage;
    p.cinPad = isrConvCinPad(Cin); p.coutPad = isrConvCoutPad(Cout);
    p.tilesX = (W + TW - 1) / TW; p.tilesY = (H + TH - 1) / TH;
    p.act = act; p.slope = slope;
    ISR_DIAG_SET(p.dbg, g_conv_dbg);
    ISR_DIAG_SET(p.stamps, g_conv_stamps);
    const long long nwg = (long long)N * p.tilesX * p.tilesY;
    if (nwg > 0x7fffffffLL) return -1;
    const dim3 block(NTHREADS);
    hipStream_t s = (hipStream_t)stream;
    static float* zero_bias = nullptr;   // bias == NULL -> a device buffer of zeros (keeps the epilogue branch-free)
    if (!bias) {
        if (!zero_bias) {
            if (hipMalloc(&zero_bias, 4096 * sizeof(float)) != hipSuccess) return -2;
            if (hipMemset(zero_bias, 0, 4096 * sizeof(float)) != hipSuccess) return -2;
        }
        if (Cout > 4096) return -1;
        p.bias = zero_bias;
    }
    using FwdKernel = void (*)(ConvParams);
    const int ups = upsample2x ? 1 : 0;        // what an upsampling variant's id is ahead of the plain one's
    const int which = upsample2x ? 0 : 1;      // index into the kernel tables (upsampling first: the order the instantiations have in the code object)
    p.cgroups = 1;
#ifdef ISR_DIAG
    if (g_conv_algo != 1) {
        // one workgroup per CU: one launch per group of up to 64 output channels (2 M tiles per wave)
        isr_lds_opt_in<conv3x3_fwd_kernel<1, true>, conv3x3_fwd_kernel<1, false>>((int)conv_fwd_lds_bytes<1>());
        isr_lds_opt_in<conv3x3_fwd_kernel<2, true>, conv3x3_fwd_kernel<2, false>>((int)conv_fwd_lds_bytes<2>());
        static const FwdKernel whole[2][2] = { { conv3x3_fwd_kernel<1, true>, conv3x3_fwd_kernel<1, false> }, { conv3x3_fwd_kernel<2, true>, conv3x3_fwd_kernel<2, false> } };
        for (int co0 = 0; co0 < p.coutPad; co0 += 64) {
            p.co0 = co0;
            const int mt = (p.coutPad - co0 == 32) ? 1 : 2;
            const int cg = Cout - co0 < 64 ? Cout - co0 : 64;
            const int rc = isr_launch(mt * 2 + ups, 2.0 * 9 * Cin * cg * (double)N * H * W, whole[mt - 1][which], dim3((unsigned)nwg), block,
                                      mt == 1 ? conv_fwd_lds_bytes<1>() : conv_fwd_lds_bytes<2>(), s, p);
            if (rc) return rc;
        }
        return 0;
    }
#endif
    // two workgroups per CU, one 32-channel group each; the grid covers all groups of all tiles
    // (> 64 KiB of dynamic LDS needs an explicit opt-in)
    isr_lds_opt_in<conv3x3_fwd2_kernel<true, 4>, conv3x3_fwd2_kernel<false, 4>>((int)conv_fwd2_lds_bytes<4>());
    p.co0 = 0;
    p.cgroups = p.coutPad / 32;
    if (nwg * p.cgroups > 0x7fffffffLL) return -1;
    // small problems: 4x32 tiles (one row per wave) when the 16x32 tiling would leave most of the 2 x #CU slots empty
    const long long tilesY4 = (H + 3) / 4, nwgSmall = (long long)N * p.tilesX * tilesY4 * p.cgroups;
    const bool small = (g_conv_tile == 1) || (g_conv_tile == 0 && nwg * p.cgroups < 384 && nwgSmall <= 0x7fffffffLL);
    // smaller still (at most one 4x32 workgroup per CU): one output row per workgroup, K split over its waves
    const long long nwgRow = (long long)N * H * p.tilesX * p.cgroups;
    const bool rows = !upsample2x && nwgRow <= 0x7fffffffLL &&
                      ((g_conv_tile == 3) || (g_conv_tile == 0 && small && nwgSmall <= g_row_threshold));
    static const FwdKernel tile4[2] = { conv3x3_fwd2_kernel<true, 1>, conv3x3_fwd2_kernel<false, 1> };
    static const FwdKernel tile16[2] = { conv3x3_fwd2_kernel<true, 4>, conv3x3_fwd2_kernel<false, 4> };
    FwdKernel kernel = tile16[which];
    int variant = 8 + ups;
    long long groups = nwg * p.cgroups;
    size_t lds = conv_fwd2_lds_bytes<4>();
    if (rows) {
        kernel = conv3x3_rowsplit_kernel; variant = ROW_VARIANT; groups = nwgRow; lds = 0;
    } else if (small) {
        p.tilesY = (int)tilesY4;
        kernel = tile4[which]; variant = 10 + ups; groups = nwgSmall; lds = conv_fwd2_lds_bytes<1>();
    }
    return isr_launch(variant, 2.0 * 9 * Cin * Cout * (double)N * H * W, kernel, dim3((unsigned)groups), block, lds, s, p);
}

}  // extern "C"
