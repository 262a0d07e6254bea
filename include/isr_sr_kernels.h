/*
 * isr_sr_kernels.h -- C-ABI of libisr_sr.so: the hand-written gfx950 kernels behind the
 * super-resolution network (EnhanceNet) of the reference.
 *
 * The reference has no native interface on this path: its convolutions are `nn.Conv2d`
 * modules dispatched to cuDNN through PyTorch (SuperresolutionNetwork/models/enhancenet.py:92-125,
 * forward :136-144).  These entry points are what a maintainer binds in place of those library
 * calls: plain device pointers, sizes and a hipStream_t -- no torch types.
 *
 * All tensors are fp32, NCHW, contiguous, resident on the current HIP device.
 * Every function returns 0 on success, a negative value on invalid arguments or launch failure.
 */
#ifndef ISR_SR_KERNELS_H
#define ISR_SR_KERNELS_H

#ifdef __cplusplus
extern "C" {
#endif

/* activation codes */
#define ISR_ACT_NONE 0
#define ISR_ACT_RELU 1
#define ISR_ACT_LEAKY 2   /* LeakyReLU / single-parameter PReLU with slope `slope` */
#define ISR_ACT_GATE 3    /* isrConv3x3Forward[Strided] only: y = residual > 0 ? conv + bias : 0 -- the ReLU backward of a
                             conv -> ReLU pair folded into the data-gradient launch (residual = the ReLU's output) */

/* Padded sizes of the kernel-side weight layout [9][cinPad][coutPad]. */
int isrConvCinPad(int Cin);
int isrConvCoutPad(int Cout);

/* Re-lays PyTorch conv weights w[Cout][Cin][3][3] into wprep[9][cinPad][coutPad] (zero padded).
 * transpose_flip = 0: forward weights,  tap = ky*3+kx, wprep[tap][ci][co] = w[co][ci][ky][kx].
 * transpose_flip = 1: data-gradient weights (the roles of Cin/Cout swap and the taps flip):
 *   wprep[tap][co][ci] = w[co][ci][2-ky][2-kx], sized [9][isrConvCinPad(Cout)][isrConvCoutPad(Cin)]. */
int isrConvPrepareWeights(const float* w, float* wprep, int Cout, int Cin, int transpose_flip, void* stream);

/* Fused 3x3 convolution, stride 1, zero padding 1 (replaces nn.Conv2d(...,3,padding=1) + nn.ReLU
 * (+ the residual add of enhancenet.py:141, + the preceding nn.Upsample(x2, bilinear) of :116,:119)):
 *     y = act(conv3x3(U(x), w) + bias) + residual
 * x: [N][Cin][H/u][W/u] with u = 2 if upsample2x (bilinear, align_corners=False) else 1;
 * wprep: from isrConvPrepareWeights(.., 0); bias: [Cout] or NULL; residual: [N][Cout][H][W] or NULL;
 * y: [N][Cout][H][W].  H, W are the OUTPUT sizes. */
int isrConv3x3Forward(const float* x, const float* wprep, const float* bias, const float* residual, float* y,
                      int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x, void* stream);

/* The same convolution on tensors whose channel planes are not packed: x / y / residual are addressed as
 * base + n * image + c * plane + row * cols + col (strides in floats; plane >= rows * cols; one image must
 * stay below 2 GiB).  Lets a caller pad the plane size of the 1080p activations: with a plane of exactly
 * 1920 x 1080 x 4 B the 64 planes alias in the memory system and the conv loses ~15 %. */
int isrConv3x3ForwardStrided(const float* x, const float* wprep, const float* bias, const float* residual, float* y,
                             int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x,
                             long long xPlane, long long xImage, long long yPlane, long long yImage,
                             long long rPlane, long long rImage, void* stream);

/* The same fused convolution for Cout <= 8 (EnhanceNet's final 64 -> 6 layer, enhancenet.py:124) on
 * 4x4x1 MFMA blocks (4 channels x 64 pixels per instruction) instead of the 32-row MFMA tile.
 * isrConvSmallPrepare re-lays w[Cout][Cin][3][3] into w8 (isrConvSmallWeightFloats(Cin) floats, a layout
 * private to the kernel) and bias into bias8[8] (zero padded); no upsampling variant.
 * isrConvSmallCinPad is kept for callers that sized buffers with it (Cin rounded up to 8). */
int isrConvSmallCinPad(int Cin);
long long isrConvSmallWeightFloats(int Cin);
int isrConvSmallPrepare(const float* w, const float* bias, float* w8, float* bias8, int Cout, int Cin, void* stream);
int isrConv3x3SmallCout(const float* x, const float* w8, const float* bias8, const float* residual, float* y,
                        int N, int Cin, int H, int W, int Cout, int act, float slope, void* stream);
/* ... with a strided input (see isrConv3x3ForwardStrided); y and residual are packed. */
int isrConv3x3SmallCoutStrided(const float* x, const float* w8, const float* bias8, const float* residual, float* y,
                               int N, int Cin, int H, int W, int Cout, int act, float slope,
                               long long xPlane, long long xImage, void* stream);

/* SPLIT-OPERAND form of the same fused convolution: fp32-equivalent accuracy on the fp16 matrix pipe (the default
 * inference path; what it replaces is the cuDNN convolution behind nn.Conv2d in
 * SuperresolutionNetwork/models/enhancenet.py:92-125, as isrConv3x3Forward does).  Every fp32 operand v is split into
 * two fp16 numbers hi = RN16(v), lo = RN16(v - hi) (22 significand bits) and x*w becomes the three products
 * x_hi*w_hi + x_hi*w_lo + x_lo*w_hi on v_mfma_f32_32x32x16_f16, accumulated in fp32; the weights are pre-scaled by a
 * per-layer power of two (undone exactly in the epilogue) so that w_lo stays a normal fp16 number.  Error vs an fp64
 * convolution: that of the exact fp32 kernel.  Inputs must satisfy |x| < 65520 (larger values become inf, loudly).
 * Same tensors / strides / act / residual / upsample2x conventions as isrConv3x3ForwardF16 below; wq: prepared by
 * isrConvSplitPrepare into isrConvSplitWeightBytes(Cin, Cout) bytes of device memory (layout private to the kernel). */
long long isrConvSplitWeightBytes(int Cin, int Cout);
int isrConvSplitPrepare(const float* w, void* wq, int Cout, int Cin, void* stream);
/* The same preparation for up to isrConvSplitPrepareManyMax() layers in two launches: per layer the forward image
 * (wqForward[l], isrConvSplitWeightBytes(cin, cout) bytes, may be NULL) and the image of the data-gradient convolution
 * w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx] (wqBackward[l], isrConvSplitWeightBytes(cout, cin) bytes, may be NULL).  Training
 * re-prepares every layer after every optimizer step.  Pointer arrays are host arrays.  0 ok, -1 bad arguments, -2 launch failure. */
int isrConvSplitPrepareManyMax(void);
int isrConvSplitPrepareMany(int n, const float* const* w, void* const* wqForward, void* const* wqBackward, const int* cout, const int* cin, void* stream);
int isrConv3x3ForwardSplit(const float* x, const void* wq, const float* bias, const float* residual, float* y,
                           int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x,
                           long long xPlane, long long xImage, long long yPlane, long long yImage,
                           long long rPlane, long long rImage, void* stream);

/* HALF-PRECISION FAST MODE of the same fused convolution (inference; not the parity path -- SURVEY.md 8(d) lets a
 * reduced-precision mode be reported separately, judged by PSNR): operands rounded to fp16 (saturating) on their way
 * into LDS, v_mfma_f32_32x32x16_f16 with fp32 accumulation, fp32 tensors in memory as above (strides in floats, rows packed).  wq: prepared by
 * isrConvF16Prepare into isrConvF16WeightBytes(Cin, Cout) bytes of device memory (layout private to the kernel).
 * act: ISR_ACT_NONE / RELU / LEAKY. */
long long isrConvF16WeightBytes(int Cin, int Cout);
int isrConvF16Prepare(const float* w, void* wq, int Cout, int Cin, void* stream);
int isrConv3x3ForwardF16(const float* x, const void* wq, const float* bias, const float* residual, float* y,
                         int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x,
                         long long xPlane, long long xImage, long long yPlane, long long yImage,
                         long long rPlane, long long rImage, void* stream);
/* The same kernel with bf16 operands (same buffer sizes and calling convention; wq from isrConvBf16Prepare): the
 * mixed-precision TRAINING mode uses it for the forward and data-gradient convolutions, whose operands (gradients)
 * span the fp32 exponent range -- fp16 would flush the small ones to zero.  Both variants also accept
 * act = ISR_ACT_GATE (y = residual > 0 ? conv + bias : 0). */
int isrConvBf16Prepare(const float* w, void* wq, int Cout, int Cin, void* stream);
int isrConv3x3ForwardBf16(const float* x, const void* wq, const float* bias, const float* residual, float* y,
                          int N, int Cin, int H, int W, int Cout, int act, float slope, int upsample2x,
                          long long xPlane, long long xImage, long long yPlane, long long yImage,
                          long long rPlane, long long rImage, void* stream);
/* upsample2x = 1 (x: [N][Cin][H/2][W/2], fused bilinear x2) needs W/2 % 4 == 0, plane / image strides % 4 == 0 and a
 * 16-byte aligned x (else -3): this predicate says so beforehand. */
int isrConvF16SupportsUpsample(long long x_address, int Win, long long xPlane, long long xImage);

/* Weight gradient of the same convolution: dw[Cout][Cin][3][3] = sum_{n,y,x} gz[n][co][y][x] * x[n][ci][y+ky-1][x+kx-1]
 * and db[Cout] = sum gz.  x: [N][Cin][H][W], gz: [N][Cout][H][W] (gradient w.r.t. the pre-activation).
 * workspace: at least isrConvWeightGradWorkspace(...) bytes of device memory. dw/db are overwritten. */
long long isrConvWeightGradWorkspace(int N, int Cin, int H, int W, int Cout);
int isrConv3x3WeightGrad(const float* x, const float* gz, float* dw, float* db, void* workspace,
                         int N, int Cin, int H, int W, int Cout, void* stream);

/* The same weight (and bias) gradient summed over `segments` (<= isrConvWeightGradMaxSegments()) pairs of tensors
 * xs[k]: [N][Cin][H][W], gzs[k]: [N][Cout][H][W] in ONE pass: the T frames of a training clip
 * (SuperresolutionNetwork/mainVideoUnshaded.py:416-466) share the network's weights, so instead of T launches per
 * layer followed by T-1 accumulations the clip's weight gradient is one launch over all frames' pixels.  xs / gzs
 * are HOST arrays of device pointers (copied into the kernel arguments). */
int isrConvWeightGradMaxSegments(void);
int isrConv3x3WeightGradSegments(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                 int N, int Cin, int H, int W, int Cout, void* stream);
/* ...Split: the same sums on SPLIT operands -- every gz and x value as two fp16 numbers, three fp16 MFMAs per product,
 * fp32 accumulation (see isrConv3x3ForwardSplit): the fp32 kernel's accuracy against fp64 at 5.3x fewer matrix cycles;
 * gz is scaled by a power of two taken from its maximum over the launch (two small kernels) and unscaled exactly by the
 * slab reduction.  The training default for layers with many tiles.  W % 4 == 0 and 16-byte aligned gzs[k] (else -3 / -1).
 * ...Bf16: the same sums with bf16 MFMA operands (fp32 accumulation and results; bias gradient from the fp32 values): the
 * weight-gradient half of the opt-in mixed-precision training mode.  W % 4 == 0 and 16-byte aligned gzs[k] (else -3 / -1). */
int isrConv3x3WeightGradSegmentsSplit(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                      int N, int Cin, int H, int W, int Cout, void* stream);
/* Per-wave maxima of the NEXT isrConv3x3ForwardSplit launch (training: a data gradient that will be a weight gradient's gz operand):
 * `words` -> a zeroed device array of `capacity` words; the launch, if its kernel form supports it and 4 x its workgroups fit, leaves in
 * word 4 w + v the bit pattern of the largest |value| wave v of workgroup w stored.  isrTakeMaxSlotWords() -> the number of words the
 * last armed launch used (0: not supported / did not fit -- make the pass over the tensor instead). */
void isrSetMaxSlots(void* words, int capacity);
int isrTakeMaxSlotWords(void);
/* ...SplitMax: as ...Split, with the maxima of the gz tensors supplied: gzmax[k] (HOST array of device pointers) -> maxWords words
 * whose maximum is the bit pattern of max |gzs[k]|, as left by the kernel that produced the tensor (isrResBlockSmall's zmax /
 * ymax, isrSetMaxSlots: one word per wave); the pass over gz that ...Split makes to find its scale is skipped.
 * accumulate: bit 0 -> dw += the gradient, bit 1 -> db += (instead of =), i.e. the slab reduction adds straight into a parameter's .grad;
 * the same bits as the call followed by `grad += dw`.  gzmax == NULL and accumulate == 0: exactly ...Split. */
int isrConv3x3WeightGradSegmentsSplitMax(const float* const* xs, const float* const* gzs, const void* const* gzmax, int maxWords, int segments,
                                         float* dw, float* db, int accumulate, void* workspace, int N, int Cin, int H, int W, int Cout, void* stream);
int isrConv3x3WeightGradSegmentsBf16(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                     int N, int Cin, int H, int W, int Cout, void* stream);

/* x2 bilinear upsampling, align_corners=False (nn.Upsample(scale_factor=2, mode='bilinear') of
 * SuperresolutionNetwork/models/enhancenet.py:116,119 when it is not fused into the following convolution, i.e. in
 * training) and its adjoint.  x / gx: [planes][h][w], y / gy: [planes][2h][2w], packed; w even.  The adjoint is a
 * gather (no atomics: bitwise reproducible). */
int isrUpsample2xForward(const float* x, float* y, long long planes, int h, int w, void* stream);
int isrUpsample2xBackward(const float* gy, float* gx, long long planes, int h, int w, void* stream);

/* Residual reconstruction of the network output (SuperresolutionNetwork/models/enhancenet.py:65-78, reconType='residual'):
 * out[n][c] = y[n][c] + bilinear_x4(x[n][c]) (align_corners=False) for c < k, out[n][c] = y[n][c] for k <= c < Cout -- the
 * slice / F.interpolate / add / cat of the reference as one launch.  y, out: [N][Cout][4h][4w], x: [N][Cin][h][w], packed.
 * The backward w.r.t. y is the identity; isrReconResidualBackward writes the one w.r.t. x: gx [N][Cin][h][w], the adjoint of
 * the resize for channels < k (a gather: bitwise reproducible), zero for the others.  0 ok, -1 bad arguments, -2 launch failure. */
int isrReconResidualForward(const float* y, const float* x, float* out, int N, int Cout, int Cin, int k, int h, int w, void* stream);
int isrReconResidualBackward(const float* gy, float* gx, int N, int Cout, int Cin, int k, int h, int w, void* stream);

/* LossNetUnshaded (SuperresolutionNetwork/losses/lossnet_unshaded.py:236-388) for the l1 / mse / temp-l2 terms on
 * mask / normal / ao / depth / colour, fused: one pass forward (+ a one-workgroup reduction), one pass backward.
 * gt, pred, prev: [N][6][H][W] (mask, normal xyz, depth, ao), W % 4 == 0; prev = warped previous prediction or NULL
 * (then the temp-l2 terms are skipped).  A border of `pad` pixels is treated as zeroed in all three (the module's
 * `pad`).  weights15 / enabled bit: index kind * 5 + target, kind 0 mse, 1 l1, 2 temp-l2, target 0 mask, 1 normal,
 * 2 ao, 3 depth, 4 colour.  shading12: ambient*material, diffuse*material, light direction, background (specular
 * is off in the loss shader, lossnet_unshaded.py:116-126).  values16 (device): the 15 term means (0 for terms that
 * are not enabled) and [15] = sum of weight * mean.  workspace: isrLossUnshadedWorkspace() bytes.
 * Backward: gvalues16 (device) is d L / d values16, of which only [15] is read; writes gpred (and gprev unless
 * NULL), both [N][6][H][W].  gt, pred, prev, gpred and gprev must be 16-byte aligned (else -1, nothing is launched). */
long long isrLossUnshadedWorkspace(void);
int isrLossUnshadedForward(const float* gt, const float* pred, const float* prev, int N, int H, int W, int pad,
                           const float* weights15, unsigned enabled, const float* shading12, float ao_strength, int inverse_ao,
                           void* workspace, float* values16, void* stream);
int isrLossUnshadedBackward(const float* gt, const float* pred, const float* prev, int N, int H, int W, int pad,
                            const float* weights15, unsigned enabled, const float* shading12, float ao_strength, int inverse_ao,
                            const float* gvalues16, float* gpred, float* gprev, void* stream);

/* The downsample-consistency terms of LossNetUnshaded (SuperresolutionNetwork/losses/lossnet_unshaded.py:63-70,258-282 with
 * lossbuilder.py:343-377, `l2-ds` / `l1-ds`): loss(sample(a), sample(b)) with sample = bilinear resize by 1/4 (align_corners=False),
 * which is the mean of the centre 2 x 2 pixels (rows / columns 4i+1, 4i+2) of every 4 x 4 cell, and the mean over the low-resolution
 * tensor.  pred [N][6][H][W] (mask, normal xyz, depth, ao), input [N][5][H][W] (the upsampled low-resolution input: mask, normal xyz,
 * depth), gate g = clamp(input mask / 2 + 1/2, 0, 1):
 *   target 0 mask    a = input mask                       b = pred mask
 *          1 normal  a = input normal / max(|.|, 1e-7) g  b = pred normal / max(|.|, 1e-7) g
 *          2 depth   a = input depth g                    b = pred depth g
 *          3 colour  a = the loss shader of input, ao factor 1     b = the loss shader of pred (ao_strength, inverse_ao)
 * A border of `pad` pixels of pred -- NOT of input -- is treated as zeroed: such a pixel contributes the fields of six zero channels
 * (the shader of a zero pixel is not 0) and receives no gradient.  weights8 / enabled bit: index kind * 4 + target, kind 0 l2, 1 l1.
 * shading12, ao_strength, inverse_ao as isrLossUnshadedForward takes them.  isrLossDownsampleSupported: H % 4 == 0, W % 4 == 0 and
 * 2 pad < min(H, W).  pred, input and gpred must be 16-byte aligned (else -1, nothing is launched).
 * Forward: values8 (device) = the eight means (0 for terms that are not enabled); *total (device, in/out) += sum of weight * mean, so
 * that the call continues the total that isrLossUnshadedForward wrote on the same stream.  workspace: isrLossDownsampleWorkspace()
 * bytes.  Two launches, no atomics, nothing read on the host: the same bits on every run, and capturable.
 * Backward: gtotal (device) is d L / d total; ADDS d L / d pred of the enabled terms into gpred [N][6][H][W] at the four centre pixels
 * of every cell that lie inside the border and touches no other element -- on the stream on which isrLossUnshadedBackward has written
 * gpred, or after a zero fill.  l1: sgn(0) = 0; clamps, |x|' and the normalisation as in isrLossUnshadedBackward.
 * 0 ok, -1 bad arguments, -2 launch failure. */
int isrLossDownsampleSupported(int N, int H, int W, int pad);
long long isrLossDownsampleWorkspace(void);
int isrLossDownsampleForward(const float* pred, const float* input, int N, int H, int W, int pad, const float* weights8, unsigned enabled,
                             const float* shading12, float ao_strength, int inverse_ao, void* workspace, float* values8, float* total,
                             void* stream);
int isrLossDownsampleBackward(const float* pred, const float* input, int N, int H, int W, int pad, const float* weights8, unsigned enabled,
                              const float* shading12, float ao_strength, int inverse_ao, const float* gtotal, float* gpred, void* stream);

/* Inputs of the discriminators of the adversarial terms (SuperresolutionNetwork/losses/lossnet_unshaded.py:313-354, :414-495), one
 * launch each way.  out [N][C][H][W] = the parts that are present in the order in_a, in_b ([N][5][H][W], the upsampled input and the
 * warped previous input, or NULL), part8(cur), part8(prev) (cur, prev [N][6][H][W]; prev or NULL): C = 26 (all four), 16 (cur + prev)
 * or 13 (in_a + cur), any other combination returns -1.  part8(x) = mask, normal / max(|normal|, 1e-7), then colour rgb, ao
 * (order 0, the generator side) or ao, colour rgb (order 1, train_discriminator).  The colour is the loss shader (shading12,
 * ao_strength, inverse_ao as isrLossUnshadedForward takes them; no specular, no gate) of the normalised normal, for cur with
 * cur_raw_normal != 0 of the normal as it arrives.  Every channel of a pixel within `pad` of the border is 0 (the module's pad, shade,
 * pad again), so the operands are passed unpadded.  isrDiscrInputSupported: W % 4 == 0 and 2 pad < min(H, W); every pointer must be
 * 16-byte aligned (else -1).
 * Backward: gout [N][C][H][W] is d L / d out, C names its layout; writes gcur (and gprev unless NULL), [N][6][H][W], 0 at border
 * pixels.  The inputs get no gradient.  Clamps pass their gradient inclusive at 0 and 1, |x|' = 0 at 0, the normalisation gives
 * g / 1e-7 where |normal| <= 1e-7 (the conventions of isrLossUnshadedBackward).  No atomics: the same bits on every run. */
int isrDiscrInputSupported(int N, int H, int W, int pad);
int isrDiscrInputForward(const float* in_a, const float* in_b, const float* cur, const float* prev, float* out, int N, int H, int W, int pad,
                         int order, int cur_raw_normal, const float* shading12, float ao_strength, int inverse_ao, void* stream);
int isrDiscrInputBackward(const float* cur, const float* prev, const float* gout, float* gcur, float* gprev, int C, int N, int H, int W, int pad,
                          int order, int cur_raw_normal, const float* shading12, float ao_strength, int inverse_ao, void* stream);

/* Recurrent network input of a training clip for frames t > 0 (SuperresolutionNetwork/mainVideoUnshaded.py:436-447,
 * 463-466 with models/videotools.py:8-25,51-87), fused:
 *   previous_output = cat(clamp(p0,-1,1), normalize(p1..3), clamp(p4,0,1), clamp(p5,0,1))   p = prev_raw [B][6][4h][4w]
 *   warped    [B][6][4h][4w] = warp_upscale(previous_output, flow, 4, special_mask=True)
 *   net_input [B][101][h][w] = cat(input, flatten_high(warped, 4))
 * input: [B][5][h][w], flow: [B][2][h][w], both with an explicit batch stride in floats (views of [B][T][..] clips).
 * Backward: g_net_input / g_warped (either may be NULL) -> g_prev_raw; scratch: B*6*4h*4w floats (the gradient of
 * previous_output, accumulated with float atomics like PyTorch's grid_sampler backward). */
int isrRecurrentInputForward(const float* prev_raw, const float* input, const float* flow, float* net_input, float* warped,
                             int B, int h, int w, long long inputBatchStride, long long flowBatchStride, void* stream);
int isrRecurrentInputBackward(const float* prev_raw, const float* flow, const float* g_net_input, const float* g_warped,
                              float* scratch, float* g_prev_raw, int B, int h, int w, long long flowBatchStride, void* stream);

/* One step of Adam (torch.optim.Adam as mainVideoUnshaded.py:287-289 uses it: betas (0.9, 0.999), eps 1e-8, no weight decay) over
 * FLAT buffers of n floats: params -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps) with the moments updated first;
 * step[0] (device float) = steps taken so far, incremented by the call.  lr_dev (device, may be NULL) overrides lr.  The betas are
 * doubles in (0, 1) (else -1): 1 - beta and the bias corrections are formed in double, as torch.optim.Adam forms them. */
int isrAdamFlatStep(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long long n, const float* lr_dev, float lr,
                    double beta1, double beta2, float eps, float* step, void* stream);

/* gz = gy * act'(y) for the activations above (y is the post-activation output, before the residual add).  16-byte accesses where all
 * three pointers are 16-byte aligned, dword accesses otherwise: the same bits. */
int isrActBackward(const float* gy, const float* y, float* gz, long long count, int act, float slope, void* stream);

/* Input assembly of one inference frame (replaces inference/loadedmodel.py:84-118,
 * models/videotools.py:8-25,51-87 and utils/initial_image.py:5-54 as ~60 PyTorch launches):
 * net_input[101][h][w] = cat(mask*2-1, normal, depth  from the renderer's HWC G-buffer,
 *                           flatten_high(warp_upscale(prev_high, flow, 4, special_mask=True), 4)).
 * flow_filled: [2][h][w] hole-filled flow; prev_high: [6][4h][4w] or NULL, in which case init_mode
 * selects initialImage: 0 "zero", 1 "unshaded", 2 "input". */
int isrAssembleInput(const float* gbuffer_hwc12, const float* flow_filled, const float* prev_high, float* net_input,
                     int h, int w, int init_mode, int ao_inverted, void* stream);
/* ... rows [row0, row1) of it only (the other rows of net_input are left as they are): a rank that super-resolves a screen strip
 * assembles its strip + halo instead of the whole frame (parallel_sr.py). */
int isrAssembleInputRows(const float* gbuffer_hwc12, const float* flow_filled, const float* prev_high, float* net_input,
                         int h, int w, int init_mode, int ao_inverted, int row0, int row1, void* stream);
/* ... and of a rectangle rows [row0, row1) x columns [col0, col1) only: a rank that super-resolves a screen TILE + halo
 * (parallel_sr.StripSuperResolution with a rows x columns grid). */
int isrAssembleInputRect(const float* gbuffer_hwc12, const float* flow_filled, const float* prev_high, float* net_input,
                         int h, int w, int init_mode, int ao_inverted, int row0, int row1, int col0, int col1, void* stream);
/* ... the whole frame straight into the dataflow trunk's workspace: the 101 channels leave PACKED-SPLIT, where isrTrunkDataflow's own packing
 * pass would have put them (isrTrunkDataflowInputLayout(101, h, w)), together with that pass's housekeeping (the planes' zero units, the
 * tiles' progress counters); the launch that follows on the same stream is isrTrunkDataflowPrepacked.  Same values, same split: the
 * trunk's result is bit-identical.  Of net_input ([101][h][w] as above) only channels 0 .. 4 are written (what isrFinishFrame / the fused
 * tail read back); channels 5 .. 100 stay UNDEFINED.  -3: the trunk does not take this size. */
int isrAssembleInputPacked(const float* gbuffer_hwc12, const float* flow_filled, const float* prev_high, float* net_input,
                           int h, int w, int init_mode, int ao_inverted, void* trunk_workspace, void* stream);

/* Input assembly of one frame of a COLOUR network (RGB in, RGB out; SuperresolutionNetwork/inference/loadedmodel.py:97-118), one launch:
 *   net_input[variant + 48][h][w] = cat(selection of the G-buffer, flatten_high(warp_upscale(prev_high3, flow, 4, special_mask=False), 4))
 * variant = number of selected channels: 8 clamp(r g b mask nx ny nz depth, 0, 1); 7 r g b mask nx ny nz; 5 r g b mask depth; 4 r g b mask.
 * prev_high3: [3][4h][4w] (the previous frame's clamped output) or NULL; then init_mode 0 gives zeros and init_mode 2 the x4 bilinear
 * resize of the selection's first three planes, which is warped by the flow like any previous image (so flow_filled is needed on the
 * first frame as well).  init_mode 1 ("unshaded") does not exist for three channels: -1.  The warp's arithmetic is isrAssembleInput's
 * (all three channels zero-padded, no mask remap): bit-identical to models/videotools.py. */
int isrAssembleInputColour(const float* gbuffer_hwc12, const float* flow_filled, const float* prev_high3, float* net_input,
                           int h, int w, int variant, int init_mode, void* stream);

/* Hole filling of the low-res flow (channels 8,9 of the HWC G-buffer) where the mask (channel 3) is 0:
 * mask-weighted push-pull pyramid, the on-device replacement of the reference's CPU OpenCV
 * cv.inpaint call (inference/loadedmodel.py:77-82).  flow_out: [2][h][w].  Three launches. */
long long isrFlowFillWorkspace(int h, int w);
int isrFlowFill(const float* gbuffer_hwc12, float* flow_out, void* workspace, int h, int w, void* stream);
/* ... with `threads` (64..1024, a power of two) per workgroup of the two grid-wide launches instead of 1024 (the
 * single-workgroup pyramid pass in between always uses 1024).  256 = one wave per SIMD: the three
 * launches then fit beside the SR network's conv workgroups when the fill of the NEXT frame runs on a side stream
 * (1024-thread workgroups evict conv workgroups from their CU and cost the network more than the fill takes). */
int isrFlowFillEx(const float* gbuffer_hwc12, float* flow_out, void* workspace, int h, int w, int threads, void* stream);
/* The same result (bit for bit) in ONE launch: a workgroup per 64 x 64 tile pulls its own part of levels 1 .. 6 in LDS, the workgroup
 * that arrives last finishes the few cells above, every tile pushes back down on regions widened by the bilinear footprint
 * (csrc/sr_frame.hip: flow_fill_one_kernel).  `workspace` (isrFlowFillWorkspace bytes) must have been ZERO-FILLED ONCE before its first
 * use here (launch tickets live in it) and serves one stream at a time.  isrFlowFillOneSupported: images of at most 256 tiles (the
 * workgroups wait for one another inside the launch); otherwise -1 and the caller uses isrFlowFillEx.  A workgroup that waited
 * longer than 50 ms gives up and sets the error word (isrSetFlowFillErrorWord; default: a word of the workspace) -- never a hang. */
int isrFlowFillOneSupported(int h, int w);
int isrFlowFillOne(const float* gbuffer_hwc12, float* flow_out, void* workspace, int h, int w, void* stream);
void isrSetFlowFillErrorWord(unsigned* word);

/* End of one inference frame: raw[6][4h][4w] (EnhanceNet output before its residual reconstruction)
 * -> next_prev = cat(clamp(mask +- 1), normalize(normal), clamp(depth, ao in [0,1])) after
 * out[:5] += bilinear x4 of net_input[:5] (models/enhancenet.py:65-78, mainGUI.py:594-599), and
 * rgb[3][4h][4w] = ScreenSpaceShading(next_prev) (utils/shading.py:148-191; rgb may be NULL).
 * shading24: ambient[3], diffuse[3], specular[3], light(normalised)[3], material[3], background[3] (host). */
int isrFinishFrame(const float* raw, const float* net_input, float* next_prev, float* rgb, int h, int w,
                   const float* shading24, int exponent, float ao_strength, int inverse_ao, int enable_specular, void* stream);

/* The frame's last layer and isrFinishFrame in ONE launch: conv3x3(x [Cin][4h][4w], 64 -> 6) + bias feeds the per-pixel
 * finishing code directly (no [6][4h][4w] round trip through memory).  w8 / bias8 from isrConvSmallPrepare for Cout = 6;
 * x may have padded channel planes (xPlane floats apart); the other arguments are those of isrFinishFrame. */
int isrConvSmallFinishFrame(const float* x, const float* w8, const float* bias8, const float* net_input, float* next_prev, float* rgb,
                            int Cin, int h, int w, long long xPlane, const float* shading24, int exponent, float ao_strength,
                            int inverse_ao, int enable_specular, void* stream);

/* End of one frame of a COLOUR network: out3[c] = clamp(raw3[c] + bilinear x4 of net_input[c], 0, 1), c = 0 .. 2 -- the arithmetic of
 * isrReconResidualForward (k = 3), then the clamp of mainVideo.py:416.  out3 [3][4h][4w] is the displayed RGB and the next frame's
 * previous image.  isrConvSmallFinishFrameColour: the same behind the last layer (64 -> 3, w8 / bias8 from isrConvSmallPrepare with
 * Cout = 3) in one launch, as isrConvSmallFinishFrame. */
int isrFinishFrameColour(const float* raw3, const float* net_input, float* out3, int h, int w, void* stream);
int isrConvSmallFinishFrameColour(const float* x, const float* w8, const float* bias8, const float* net_input, float* out3,
                                  int Cin, int h, int w, long long xPlane, void* stream);

/* isrConv3x3ForwardSplit for one image whose result is written PACKED-SPLIT instead of fp32: every output value already as
 * the (hi, lo') fp16 pair the next split-operand layer multiplies, eight channels of a pixel per 16-byte unit,
 * ps[part: hi | lo][Cout / 8][psPlane units] (unit index y W + x; Cout a multiple of 8; no residual).  The consumer
 * (isrConvTailFinishFramePacked) stages it by LDS-DMA -- the numbers are those a consumer of the fp32 tensor would form on
 * its way in, so results do not change.  ps: 2 * (Cout / 8) * psPlane * 16 bytes, 16-byte aligned.  Returns as above. */
int isrConv3x3ForwardSplitPacked(const float* x, const void* wq, const float* bias, void* ps, int Cin, int H, int W, int Cout,
                                 int act, float slope, int upsample2x, long long xPlane, long long psPlane, void* stream);

/* ... and the consumer side for plain layers: the split-operand convolution of a PACKED-SPLIT input xps (Cin / 8 groups, xpsPlane
 * units per plane, one image), result as isrConv3x3ForwardSplit (y fp32, planes yPlane floats apart, optional residual with rPlane)
 * or, with packed_out != 0, packed-split again (y = ps, yPlane = its plane stride in units, no residual). */
int isrConv3x3ForwardSplitFromPacked(const void* xps, const void* wq, const float* bias, const float* residual, void* y, int packed_out,
                                     int Cin, int H, int W, int Cout, int act, float slope, long long xpsPlane, long long yPlane, long long rPlane,
                                     void* stream);

/* The whole low-resolution trunk of one image as ONE persistent dataflow launch (csrc/sr_conv_trunk.hip):
 *   F = relu(conv3x3(x [cin0][H][W], w[0]) + b[0]);  nblocks times  F += conv3x3(relu(conv3x3(F, w[2k+1]) + b[2k+1]), w[2k+2]) + b[2k+2]
 * (models/enhancenet.py:92-112,136-141), split-operand arithmetic, bit-identical to the per-layer launches of
 * isrConv3x3ForwardSplit.  Workgroup w owns tile w of 16 x 32 pixels through all layers and starts a layer when its 3 x 3
 * neighbourhood has finished the previous one; one workgroup per CU, all resident at once.  Up to isrTrunkDataflowMaxTiles() tiles a
 * workgroup owns ONE tile (residual stream in registers, half of every hand-over through LDS); larger images (ISR_TRUNK_MT, default on)
 * take trunk_mt_kernel: a workgroup owns every #CUs-th tile and keeps the residual stream in y.  isrTrunkDataflowSupported says whether
 * these tensors qualify.  Between the layers the activations live in the workspace in the packed-split format.
 *   x: planes xPlane floats apart (rows contiguous); y (the result F): [64][H][W], planes `plane` floats apart;
 *   wq[l]: isrConvSplitPrepare images, bias[l]: [64] device or NULL, l = 0 .. 2 nblocks;
 *   workspace: isrTrunkDataflowWorkspaceBytes(cin0, H, W) bytes of device memory, 256-byte aligned, ZERO-FILLED by the caller before
 *   its first use.  Bytes 16 .. hold the tiles' progress counters and then an error word: 1 + layer if a tile's wait timed out after
 *   50 ms in ANY launch since the caller last reset it (the launches never clear it).
 * 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported shape / alignment / too many tiles. */
int isrTrunkDataflowMaxTiles(void);
long long isrTrunkDataflowWorkspaceBytes(int cin0, int H, int W);
int isrTrunkDataflowSupported(const float* x, int cin0, int H, int W, long long xPlane, long long plane);
int isrTrunkDataflow(const float* x, int cin0, long long xPlane, float* y, long long plane, const void* const* wq,
                     const float* const* bias, int nblocks, int H, int W, void* workspace, void* stream);
/* The same launch for an input that is ALREADY packed-split in the workspace (isrAssembleInputPacked on the same stream): no packing pass.
 * isrTrunkDataflowInputLayout: byte offsets into the workspace of the launch's three packed-split tensors (input, F, T; planes of
 * ((H W + 8) & ~7) 16-byte units, [hi | lo'][groups]), the input's channel groups of 8, the number of tiles. */
int isrTrunkDataflowInputLayout(int cin0, int H, int W, long long* offsets3, int* groups0, int* tiles);
int isrTrunkDataflowPrepacked(int cin0, float* y, long long plane, const void* const* wq, const float* const* bias, int nblocks, int H, int W,
                              void* workspace, void* stream);
/* Where every LATER isrTrunkDataflow launch reports a timed-out wait instead of the workspace's own word (same encoding, sticky until
 * the caller clears it; NULL restores the workspace word): one device word the caller can mirror to the host once per frame together
 * with the range-guard words (isrSetRangeFlag), so that a disturbed launch is noticed a frame later, not whenever somebody looks. */
void isrSetTrunkErrorWord(unsigned* word);

/* One residual block of the trunk, y = x + conv2(relu(conv1(x) + bias1)) + bias2 (64 -> 64 -> 64 channels, one image;
 * models/enhancenet.py:18-33,108-112,139-141), in ONE launch on the split-operand arithmetic: the same products in the same
 * order as two calls of isrConv3x3ForwardSplit (bit-identical result).  The intermediate tensor stays in a per-workgroup
 * scratch (`workspace`, isrResBlockSplitWorkspaceBytes() bytes) as LDS-ready (hi, lo) units and is streamed back by LDS-DMA.
 *   x, y: [64][H][W] fp32, 16-byte aligned, planes xPlane / yPlane floats apart (multiples of 4), W a multiple of 4;
 *   wq1 / wq2: isrConvSplitPrepare(w [64][64][3][3]); bias1 / bias2: [64] device (may be NULL).
 * isrResBlockSplitSupported -> 1 if these tensors can be taken.  0 ok, -1 bad arguments, -2 launch failure, -3 unsupported. */
/* Two chained 64 -> 64 convolutions of a BATCH OF SMALL IMAGES (W <= 32, e.g. the 32 x 32 crops of mainVideoUnshaded.py's training
 * step) in ONE launch -- a residual block, z = relu(conv(x, wa) + ba), y = conv(z, wb) + bb + x (models/enhancenet.py:18-33,139-141;
 * gate == NULL), or its data gradient, z = gate > 0 ? conv(x, wa) : 0, y = conv(z, wb) + x (x = the gradient of the block's output,
 * gate = the saved relu output, wa / wb = the flipped / transposed images of the block's second / first convolution).  Bit-identical
 * to two isrConv3x3ForwardSplit launches (the intermediate's halo rows are recomputed per 2-row tile).
 *   x, gate, z, y: packed [N][64][H][W] fp32, x and y 16-byte aligned, W a multiple of 4; wa / wb: isrConvSplitPrepare(w [64][64][3][3]);
 *   ba / bb: [64] device or NULL.  isrResBlockSmallSupported -> 1 for shapes this takes (at least 64 two-row tiles).
 *   zmax / ymax (both or neither): device arrays of 4 N ceil(H / 2) words that receive, per wave, the bit pattern of max |z| / max |y| --
 *   what isrConv3x3WeightGradSegmentsSplitMax wants for a gz operand.
 * 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported shape. */
int isrResBlockSmallSupported(int N, int H, int W);
int isrResBlockSmall(const float* x, const void* wa, const float* ba, const float* gate, const void* wb, const float* bb, float* z, float* y,
                     int N, int H, int W, void* zmax, void* ymax, void* stream);

long long isrResBlockSplitWorkspaceBytes(void);
int isrResBlockSplitSupported(const float* x, int H, int W, long long xPlane, long long yPlane);
int isrResBlockSplit(const float* x, const void* wq1, const float* bias1, const void* wq2, const float* bias2, float* y, void* workspace,
                     int H, int W, long long xPlane, long long yPlane, void* stream);

/* The 1080p TAIL of the network in two launches (csrc/sr_conv_tail.hip): relu(conv3x3(x [64][4h][4w], 64 -> 64) + bias6)
 * -> conv3x3(., 64 -> 6) + bias8 -> isrFinishFrame, i.e. models/enhancenet.py:119-125 (postblock.6 .. postblock.8) followed by
 * _recon_image (:51-90) and the viewer's clamp / normalise / shading (mainGUI.py:594-603), on the split-operand arithmetic of
 * isrConv3x3ForwardSplit.  The 64-channel tensor between the two convolutions never exists in memory: the last layer is
 * evaluated per tap as a 1x1 product on the first convolution's accumulators (54 partial planes in `workspace`), and the second
 * launch adds every pixel's nine shifted partials in a fixed order and finishes the frame.
 *   wq6: isrConvSplitPrepare(w6 [64][64][3][3]); wz: isrConvTailPrepare(w8 [6][64][3][3]) into isrConvTailWeightBytes() bytes;
 *   bias6 [64] (may be NULL), bias8 [6]: device; workspace: isrConvTailWorkspaceBytes(h, w) bytes of device memory;
 *   x: 16-byte aligned, channel planes xPlane floats apart (a multiple of 4); w must be a multiple of 4.
 * isrConvTailSupported(x, h, w, xPlane) -> 1 if the launch can take these tensors (else use isrConv3x3ForwardSplit +
 * isrConvSmallFinishFrame).  Returns 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported shape / alignment. */
long long isrConvTailWeightBytes(void);
long long isrConvTailWorkspaceBytes(int h, int w);
int isrConvTailPrepare(const float* w8, void* wz, void* stream);
int isrConvTailSupported(const float* x, int h, int w, long long xPlane);
int isrConvTailFinishFrame(const float* x, const void* wq6, const float* bias6, const void* wz, const float* bias8, void* workspace,
                           const float* net_input, float* next_prev, float* rgb, int h, int w, long long xPlane,
                           const float* shading24, int exponent, float ao_strength, int inverse_ao, int enable_specular, void* stream);
/* ... with the 64-channel input PACKED-SPLIT (isrConv3x3ForwardSplitPacked, 64 channels, [4h][4w], xpsPlane units per plane). */
int isrConvTailFinishFramePacked(const void* xps, const void* wq6, const float* bias6, const void* wz, const float* bias8, void* workspace,
                                 const float* net_input, float* next_prev, float* rgb, int h, int w, long long xpsPlane,
                                 const float* shading24, int exponent, float ao_strength, int inverse_ao, int enable_specular, void* stream);

/* The tail of a COLOUR network (postblock.8 is 64 -> 3): the same two launches with THREE output channels -- 27 tap-partial rows (one
 * 32-row block of the extra product instead of two), nine S planes and end-pixel records of 54 floats instead of eighteen and 108; the
 * same split-operand arithmetic and the same fixed order of additions, ((bias + S0) + S1) + S2 with (z0 + z1) + z2 per row, so every
 * pixel is independent of where tile borders fall.  The finishing is isrFinishFrameColour's: out3 [3][4h][4w].
 *   wz: isrConvTailPrepare3(w8 [3][64][3][3]) into isrConvTailWeightBytes() bytes; bias8 [3]; workspace: isrConvTailWorkspaceBytes3(h, w);
 *   isrConvTailSupported says whether the tensors qualify, as for six channels. */
long long isrConvTailWorkspaceBytes3(int h, int w);
int isrConvTailPrepare3(const float* w8, void* wz, void* stream);
int isrConvTailFinishFrame3(const float* x, const void* wq6, const float* bias6, const void* wz, const float* bias8, void* workspace,
                            const float* net_input, float* out3, int h, int w, long long xPlane, void* stream);
int isrConvTailFinishFrame3Packed(const void* xps, const void* wq6, const float* bias6, const void* wz, const float* bias8, void* workspace,
                                  const float* net_input, float* out3, int h, int w, long long xpsPlane, void* stream);

/* PHASE-DECOMPOSED x2-upsampling convolution (csrc/sr_conv_upsp.h): y = act(conv3x3(U2(x), w) + bias) for EnhanceNet's two
 * upsampling layers (SuperresolutionNetwork/models/enhancenet.py:113-124: nn.Upsample(scale_factor=2, mode='bilinear') + Conv2d(64, 64, 3)),
 * 64 -> 64 channels, one image, input and output PACKED-SPLIT (the layout of isrConv3x3ForwardSplitPacked: [2 parts][8 groups][plane
 * units]).  U2 is linear, so the result at the high-resolution pixel (2y + py, 2x + px) is a 3 x 3 convolution of the LOW-resolution
 * image with one of four effective weight sets: no interpolation at run time, the operands are copied into LDS as the producer left
 * them.  The output's one-pixel frame (where the convolution's zero padding drops taps) is computed exactly by a small kernel of its
 * own from the fp32 weights `w`.  Same accuracy against an fp64 convolution as isrConv3x3ForwardSplit(upsample2x = 1), not the same bits.
 *   isrConvUpsPhasePrepare(w [64][64][3][3] fp32, wq, scratch, stream): wq = isrConvUpsPhaseWeightBytes() bytes (the four stacked
 *     images, one scale), scratch = isrConvUpsPhaseScratchBytes() bytes (the effective weights in fp32; may be freed once the stream
 *     has passed this call);
 *   isrConvUpsPhase(xps [64][h][wd] packed, wq, w, bias [64] or NULL, ps [64][2h][2wd] packed, h, wd, act (NONE / RELU / LEAKY), slope,
 *     xpsPlane, psPlane (units), stream).  isrConvUpsPhaseSupported(64, 64, h, wd, xpsPlane, psPlane) -> 1 if the launch takes the shape.
 * isrPackSplit: an fp32 tensor [C][H][W] (planes xPlane floats apart, C a multiple of 8) as a packed-split tensor (what a producer's
 * packed epilogue writes).  isrTrunkDataflowPackedResult: where isrTrunkDataflow leaves its result packed-split inside its workspace.
 * Return codes as isrConv3x3ForwardSplit. */
long long isrConvUpsPhaseWeightBytes(void);
long long isrConvUpsPhaseScratchBytes(void);
int isrConvUpsPhasePrepare(const float* w, void* wq, void* scratch, void* stream);
int isrConvUpsPhaseSupported(int Cin, int Cout, int h, int wd, long long xpsPlane, long long psPlane);
int isrConvUpsPhase(const void* xps, const void* wq, const float* w, const float* bias, void* ps, int h, int wd, int act, float slope,
                    long long xpsPlane, long long psPlane, void* stream);
int isrPackSplit(const float* x, void* ps, int C, int H, int W, long long xPlane, long long psPlane, void* stream);
int isrTrunkDataflowPackedResult(int cin0, int H, int W, long long* offsetBytes, long long* planeUnits);
void isrSetTrunkPackedResult(int on);      /* 1: isrTrunkDataflow also writes that packed-split result (default 0) */
/* Rows of the 16 x 32 tile per wave in the one-tile form of isrTrunkDataflow: 2 (default; eight waves, two per SIMD) or 4 (four waves of
 * 4 rows x 64 channels, one per SIMD, accumulators in AGPRs).  Same bits either way; 4 is the slower one on MI355X.
 * Environment: ISR_TRUNK_ROWS. */
void isrSetTrunkRows(int rows);

/* SPLIT-OPERAND stride-2 TRANSPOSED convolution (csrc/sr_conv_transpose.hip): what replaces the library call behind
 * nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1) + nn.LeakyReLU of the TecoGAN generator
 * (SuperresolutionNetwork/models/tecogan.py:55-59):
 *     y[co][2i + a][2j + b] = act(bias[co] + sum_ci sum_taps x[ci][i + di][j + dj] w[ci][co][ky][kx]),    a, b in {0, 1},
 * rows a = 0: (ky 1, di 0); a = 1: (ky 2, di 0), (ky 0, di 1); columns alike; input rows >= h and columns >= w contribute nothing.
 * One image, 64 -> 64 channels, fp32 planes: x [64][h][w] with planes xPlane floats apart, y [64][2h][2w] with planes yPlane floats
 * apart (rows packed).  Same arithmetic as isrConv3x3ForwardSplit (operands as fp16 (hi, lo) pairs, three fp16 MFMAs per product, fp32
 * accumulation; |x| < 65520), same range guard (isrSetRangeFlag arms the launch).
 *   isrConvTransposeSplitPrepare(w [64][64][3][3] fp32 in the ConvTranspose2d layout [ci][co][ky][kx], wq, stream): wq =
 *     isrConvTransposeSplitWeightBytes() bytes of device memory (layout private to the kernel);
 *   isrConvTranspose3x3S2ForwardSplit(x, wq, bias [64] or NULL, y, Cin, h, w, Cout, act (NONE / RELU / LEAKY), slope, xPlane, yPlane, stream):
 *     h, w are the INPUT sizes;
 *   isrConvTranspose3x3S2SplitSupported(Cin, Cout, h, w, xPlane, yPlane) -> 1 if the launch takes these tensors.
 * 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported. */
long long isrConvTransposeSplitWeightBytes(void);
int isrConvTransposeSplitPrepare(const float* w, void* wq, void* stream);
int isrConvTranspose3x3S2SplitSupported(int Cin, int Cout, int h, int w, long long xPlane, long long yPlane);
int isrConvTranspose3x3S2ForwardSplit(const float* x, const void* wq, const float* bias, float* y, int Cin, int h, int w, int Cout,
                                      int act, float slope, long long xPlane, long long yPlane, void* stream);

/* BACKWARD of that layer (training).  With z the pre-activation output, gz = gy act'(y) (the rule of isrActBackward) and the PHASE-MAJOR
 * gradient G[n][4 co + 2 a + b][i][j] = gz[n][co][2i + a][2j + b] -- low-resolution planes in the order of F.pixel_unshuffle(., 2):
 *   isrConvTransposePhaseGradient(gy [N][C][2h][2w], y (same shape; NULL with act NONE), G [N][4C][h][w], N, C, h, w, act (NONE / RELU /
 *     LEAKY), slope, stream): the activation's backward written phase-major (csrc/sr_train.hip); bit-identical to isrActBackward followed
 *     by pixel_unshuffle.  All tensors packed.
 *   data gradient gx[n][ci][i][j] = sum_{co,ky,kx} gz[n][co][2i - 1 + ky][2j - 1 + kx] w[ci][co][ky][kx] (rows / columns -1 are outside):
 *     isrConvTransposeDataGradPrepare(w [64][64][3][3] in the ConvTranspose2d layout, wq, stream): wq = isrConvTransposeDataGradWeightBytes()
 *       bytes of device memory (layout private to the kernel; NOT the forward image);
 *     isrConvTranspose3x3S2DataGradSplit(G [N][256][h][w], wq, gx [N][64][h][w], N, C = 64, h, w, stream): convt3x3s2_dgrad_split_kernel, the
 *       forward kernel's split-operand arithmetic over G, nine 64 x 64 products per low-resolution pixel, sums in a fixed order (the same
 *       bits on every run).  Honours isrSetMaxSlots (the per-wave maxima of gx) and isrSetRangeFlag.
 *     isrConvTranspose3x3S2DataGradSplitSupported(N, C, h, w) -> 1 if the launch takes these tensors (C = 64; one image of G below 2 GiB).
 *   weight / bias gradient: isrConv3x3WeightGradSegments[Split[Max]] on (x, G) as a 64 -> 256 3x3 layer; the 9 live taps of 36 are the
 *     ConvTranspose2d weight's gradient (ops.conv_transpose_weight_from_phase), gb[co] the sum of its four phase entries.
 * 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported. */
/* The TRAINING forward: N packed images in ONE launch of the same kernel (x [N][64][h][w], y [N][64][2h][2w]); a batch of small crops
 * launched image by image leaves most of the GPU idle. */
int isrConvTranspose3x3S2ForwardSplitBatch(const float* x, const void* wq, const float* bias, float* y, int N, int h, int w,
                                           int act, float slope, void* stream);
int isrConvTransposePhaseGradient(const float* gy, const float* y, float* G, int N, int C, int h, int w, int act, float slope, void* stream);
long long isrConvTransposeDataGradWeightBytes(void);
int isrConvTransposeDataGradPrepare(const float* w, void* wq, void* stream);
int isrConvTranspose3x3S2DataGradSplitSupported(int N, int C, int h, int w);
int isrConvTranspose3x3S2DataGradSplit(const float* G, const void* wq, float* gx, int N, int C, int h, int w, void* stream);

/* STRIDE-2 3x3 convolution y = act(conv2d(x, w, bias, stride = 2, padding = 1)) (csrc/sr_conv_stride2.hip): the halving layers of the
 * reference's discriminators (SuperresolutionNetwork/losses/enhancenetsmall.py, enhancenetlarge.py).  x [N][Cin][H][W], w [Cout][Cin][3][3]
 * as nn.Conv2d holds it (no prepared image), y and gz [N][Cout][H/2][W/2], all packed fp32.  Exact fp32 MFMA, every sum in a fixed order
 * (the same bits on every run); kernels take the caller's stream and allocate nothing.
 *   ...Supported: H and W even, Cin and Cout multiples of 16 from 16 to 256 (else every entry point returns -3).
 *   ...Forward: nine Cin x Cout products per output pixel, bias (may be NULL) and activation (ISR_ACT_NONE or ISR_ACT_LEAKY) in the epilogue.
 *   ...DataGrad: gx[n][ci][p][q] = sum_{co, ky, kx : p = 2i + ky - 1, q = 2j + kx - 1} gz[n][co][i][j] w[co][ci][ky][kx], by output parity
 *     (1, 2, 2 and 4 taps); gz is the gradient of the PRE-activation (isrActBackward first); gx 8-byte aligned.
 *   ...WeightGradSegments: dw[Cout][Cin][3][3] and db[Cout] (may be NULL) summed over `segments` (<= isrConvWeightGradMaxSegments()) pairs
 *     xs[k], gzs[k] (HOST arrays of device pointers), slabs of pixels reduced in slab order; workspace: ...WeightGradWorkspace(...) bytes.
 * 0 ok, -1 bad arguments, -2 launch failure, -3 unsupported. */
int isrConv3x3S2Supported(int N, int Cin, int Cout, int H, int W);
int isrConv3x3S2Forward(const float* x, const float* w, const float* bias, float* y, int N, int Cin, int H, int W, int Cout,
                        int act, float slope, void* stream);
int isrConv3x3S2DataGrad(const float* gz, const float* w, float* gx, int N, int Cin, int H, int W, int Cout, void* stream);
long long isrConv3x3S2WeightGradWorkspace(int N, int Cin, int H, int W, int Cout);
int isrConv3x3S2WeightGradSegments(const float* const* xs, const float* const* gzs, int segments, float* dw, float* db, void* workspace,
                                   int N, int Cin, int H, int W, int Cout, void* stream);

/* The DISPLAY STAGE of the viewer's frame in one launch (csrc/sr_display.hip), per high-resolution pixel: what the reference viewer does
 * between the network and the window (SuperresolutionNetwork/mainGUI.py:603-608,626-636,762-853) -- the twelve-channel image (x4
 * bilinear of the low G-buffer with the network's channels in place), background masking, the focus-of-context blend with a
 * full-resolution G-buffer (shaded here), the channel view, the temporal post-smoothing against the warped previous DISPLAYED image, and
 * an 8-bit RGBA copy.  The arithmetic is that of isosurfacesuperresolution_amd/viewer.py: compose_display, operation by operation (no
 * contraction): the same bits wherever no shading enters, 1e-4 where the focus window is shaded (as isrFinishFrame against the module path).
 * All pointers are device pointers; optional parts are NULL.  H = 4 h, W = 4 w.  Returns 0 ok, -1 bad arguments, -2 launch failure. */
#define ISR_VIEW_COLOR 0
#define ISR_VIEW_MASK 1
#define ISR_VIEW_NORMAL 2
#define ISR_VIEW_DEPTH 3
#define ISR_VIEW_AO 4
#define ISR_VIEW_FLOW 5
typedef struct IsrDisplayParams {
    const float* gbuffer;       /* [h][w][12] the renderer's low-resolution G-buffer of the frame (mask in [0, 1]) */
    const float* rgb;           /* [3][H][W] the frame's colour: the shaded network output, or a colour network's clamped prediction */
    const float* raw;           /* [6][H][W] mask, normal, depth, AO as the network left them (clamped / normalised); NULL: a colour network */
    const float* flow;          /* [2][h][w] hole-filled flow of the frame (isrFlowFill); needed by ISR_VIEW_FLOW and with `prev` */
    const float* prev;          /* [3][H][W] the previous displayed image, or NULL: no post-smoothing.  Must not be `out` */
    const float* focus;         /* [H][W][12] full-resolution G-buffer of the same camera (read inside `viewport` where focus_mask > 0), or NULL */
    const float* focus_mask;    /* [H][W] blend weight of the focus window, 1 = full-resolution render; with `focus` */
    const float* depth_bounds;  /* [2] (min, max) depth of the frame; ISR_VIEW_DEPTH */
    float* out;                 /* [3][H][W] the displayed image */
    unsigned char* out8;        /* [H][W][4] RGBA, round(clamp(out, 0, 1) * 255), A = 255; or NULL.  4-byte aligned */
    int h, w;
    int channel;                /* ISR_VIEW_* */
    int masking;                /* 1: image = background0 + (base_mask / 2 + 1 / 2) (image - background0) */
    float background0;
    float smooth_prev, smooth_cur;      /* out = smooth_prev * warp(prev) + smooth_cur * image (with `prev`) */
    int viewport[4];            /* minX, minY, maxX, maxY of the focus window in high-resolution pixels (max exclusive) */
    float shading[18];          /* ambient, diffuse, specular, light, material, background (utils.ScreenSpaceShading.packed_parameters) */
    int exponent;
    float ao_strength;
    int enable_specular;
} IsrDisplayParams;
int isrDisplayFrame(const IsrDisplayParams* params, void* stream);

/* The viewer's frame in its NON-NETWORK render modes (mainGUI.py:712-757: nearest, bilinear, bicubic, ground truth), same file.  The
 * twelve-channel image is the rendered G-buffer itself -- mask mapped to [-1, +1], colour = clamp(shading, 0, 1) evaluated at the
 * G-buffer's resolution -- interpolated x4 with all its channels (nothing is clamped afterwards: the bicubic overshoot stays), or taken as
 * it is (ISR_BASE_IDENTITY: the G-buffer is the full-resolution one).  Focus blend, channel view, post-smoothing and RGBA copy follow as
 * in isrDisplayFrame (the same device functions); there is no background masking in these modes.
 *   ISR_BASE_NEAREST / BILINEAR / BICUBIC: TWO launches -- a pre-pass over the h x w pixels writes the planes the view shows into
 *   `low_planes` (shading each low-resolution pixel once), the display launch interpolates from those planes.  ISR_VIEW_FLOW: one launch.
 *   ISR_BASE_IDENTITY: ONE launch; `gbuffer` is [H][W][12]; no focus window (it would show the same render), no post-smoothing and no
 *   flow view (NULL `prev`, `focus`; -1 otherwise).
 * The arithmetic is isosurfacesuperresolution_amd/viewer.py: compose_baseline (models/videotools.py: upscale_nearest, upscale_bilinear,
 * upscale_bicubic), operation by operation: the same bits wherever no shading enters.  Returns as isrDisplayFrame. */
#define ISR_BASE_NEAREST 0
#define ISR_BASE_BILINEAR 1
#define ISR_BASE_BICUBIC 2
#define ISR_BASE_IDENTITY 3
typedef struct IsrDisplayBaselineParams {
    const float* gbuffer;       /* [h][w][12] the G-buffer rendered for this frame (mask in [0, 1]); ISR_BASE_IDENTITY: [H][W][12] */
    float* low_planes;          /* [12][h][w] workspace of the pre-pass (the planes of the view are written); not with ISR_BASE_IDENTITY / ISR_VIEW_FLOW */
    const float* flow;          /* as IsrDisplayParams from here on */
    const float* prev;
    const float* focus;
    const float* focus_mask;
    const float* depth_bounds;  /* [2] (min, max) depth of `gbuffer`, whichever resolution it has; ISR_VIEW_DEPTH */
    float* out;
    unsigned char* out8;
    int h, w;                   /* the LOW resolution in every mode: H = 4 h, W = 4 w */
    int mode;                   /* ISR_BASE_* */
    int channel;                /* ISR_VIEW_* */
    float smooth_prev, smooth_cur;
    int viewport[4];
    float shading[18];          /* needed by ISR_VIEW_COLOR (every mode) and by the focus window */
    int exponent;
    float ao_strength;
    int enable_specular;
} IsrDisplayBaselineParams;
int isrDisplayBaselineFrame(const IsrDisplayBaselineParams* params, void* stream);

/* The metric stage of the statistics harness (csrc/sr_metrics.hip; stats.Statistics(metrics="hip")): masked squared error (PSNR), the
 * MS-SSIM terms and the absolute-difference histogram of one image pair, as utils/psnr.py, utils/ssim.py and np.histogram define them.
 * Images: fp32 [C][H][W] as pointer + row pitch + plane pitch (in floats; the harness passes border-cropped views), every pixel widened
 * to fp64 and ALL arithmetic in fp64, operation by operation as the Python definition and with no contraction into FMAs.  `mask` /
 * `blend`: an optional fp64 plane [H][W] (row pitch in doubles), NULL = none.  `blend` replaces image a by a' = b + m (a - b) first.
 * Results stay on the device, no entry point synchronises; sums are per-workgroup partial sums in a fixed order followed by a
 * fixed-order final sum (no floating-point atomics): two calls give the same bits.  Every entry point returns 0, -1 on arguments it
 * refuses (nothing launched), -2 if a launch failed.
 *
 * isrMetricsSqErr: out[0] = sum over c, y, x of (m a - m b)^2 (this order, utils/psnr.py:13; m = 1 without a mask), out[1] = sum of m over
 *   y, x (H W without a mask).  `workspace`: ISR_METRICS_SQERR_WORKSPACE_BYTES.
 * isrMetricsMsssim: out[0..4] = mean of the SSIM map of levels 0..4, out[5..9] = mean of v1 / v2 of the same levels
 *   (utils/ssim.py: ssim(full=True): window k = min(11, H, W) of the level, valid convolution, C1 / C2 from the dynamic range guessed from
 *   image a' of the level, avg_pool2d(2) between levels), out[10] = prod over i < 4 of (out[5 + i]^w_i out[4]^w_4) (utils/ssim.py:62).
 *   `windows`: fp64 [5][121], row l = the k x k table utils.ssim.create_window(k) makes for level l (fp32 products widened), applied as a
 *   full k x k sum.  H, W >= 32 (the definition pools five times).  The level's min / max reaches the SSIM launch through `workspace`
 *   (isrMetricsMsssimWorkspace bytes; a pure size query): no host read between levels.
 * isrMetricsAbsDiffHistogram: counts[0..bins-1] = np.histogram(scale * sum over c of |a'_c - b_c|, bins, range=(0, 1)) (channels summed
 *   left to right: (d0 + d1) + d2), counts[bins] = the number of values inside [0, 1].  Values outside (and NaN) are dropped, 1.0 falls
 *   into the last bin, the index floor(v bins) is corrected against `edges` = fp64 np.linspace(0, 1, bins + 1).  bins <= 1024. */
#define ISR_METRICS_SQERR_WORKSPACE_BYTES 16384
int isrMetricsSqErr(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                    const double* mask, long long maskRow, int C, int H, int W, void* workspace, double* out, void* stream);
long long isrMetricsMsssimWorkspace(int C, int H, int W);
int isrMetricsMsssim(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                     const double* blend, long long blendRow, int C, int H, int W, const double* windows, void* workspace, double* out,
                     void* stream);
int isrMetricsAbsDiffHistogram(const float* a, long long aRow, long long aPlane, const float* b, long long bRow, long long bPlane,
                               const double* blend, long long blendRow, int C, int H, int W, double scale, int bins, const double* edges,
                               long long* counts, void* stream);

/* The pieces of the RCAN generator (models/rcan.py) that are not convolutions (csrc/sr_attention.hip).  Tensors are fp32 with packed rows,
 * addressed as base + n * image + c * plane + y * W + x (strides in floats, plane >= H W: the pad behind a plane is never read); C = 64
 * channels with R = 4 reduced channels, one image below 2 GiB, N <= 65535: anything else returns -3 (the ...Supported predicates say so
 * beforehand).  Returns: 0, -1 bad arguments, -2 launch failure, -3 unsupported.  16-byte accesses where base addresses and strides are
 * multiples of 16 bytes, a per-element path otherwise.
 *
 * Channel attention of a residual block, y = x + t * s[c] with s = sigmoid(Wu leaky(Wd mean_hw(t) + bd) + bu), in two launches:
 *   isrChannelPool: workspace[n][c][s] (double, S = isrChannelPoolSlabs(N, H, W) slabs per plane; S fills the chip at 480 x 270 and is 1
 *     for small planes) = the sum of slab s of plane (n, c) of t, accumulated in fp64 in a fixed order: the same bits on every run, no
 *     floating-point atomics.  isrChannelPoolMean: mean[n][c] = (float)(sum of the S partials in index order / (H W)) -- the value
 *     the gate below forms itself.
 *   isrChannelGateScaleAdd: every workgroup sums the S partials of its image in index order, forms the fp32 mean z[64], computes
 *     a[j] = fmaf-chain over c of Wd[j][c] z[c] starting from bd[j]; g = a > 0 ? a : a * slope; u = fmaf-chain over j of Wu[c][j] g[j]
 *     starting from bu[c]; s = 1 / (1 + expf(-u)), and stores y = x + t * s as a separately rounded multiply and add (given s, the bits of
 *     `x + t * s` in PyTorch).  wDown [4][64], bDown [4], wUp [64][4], bUp [64] as nn.Linear stores them.  `gate`: [N][64] receives s, or
 *     NULL.  Range guard: a launch armed by isrSetRangeFlag reports the largest |y| it stores, one atomic per wave.
 * The tail, out [N][Cout <= 8][4h][4w] = conv3x3(pixel_shuffle(f [N][64][h][w], 4), weight [Cout][4][3][3], zero padding 1) + bias
 * (NULL: none), clamped to [0, 1] if `clamp`, in ONE launch (isrShuffleTailColour): channel 16 c + 4 i + j of low-resolution pixel (y, x)
 * is channel c at (4 y + i, 4 x + j); the low-resolution tile and its one-pixel halo are staged in LDS, the four-channel high-resolution
 * tensor never exists in memory.  Per output value one fp32 fmaf chain starting from the bias, over (ci, ky, kx) in this nesting, zeros
 * outside the image: the value does not depend on where tile borders fall. */
int isrChannelPoolSlabs(int N, int H, int W);
int isrChannelPoolSupported(int N, int C, int H, int W, long long plane, long long image);       /* one tensor with these strides */
int isrChannelGateScaleAddSupported(int N, int C, int R, int H, int W, long long plane, long long image);       /* each of x, t, y */
int isrChannelPool(const float* t, long long tPlane, long long tImage, int N, int C, int H, int W, int S, double* workspace, void* stream);
int isrChannelPoolMean(const double* workspace, int N, int C, int H, int W, int S, float* mean, void* stream);
int isrChannelGateScaleAdd(const float* x, const float* t, float* y, long long xPlane, long long xImage, long long tPlane, long long tImage,
                           long long yPlane, long long yImage, const double* workspace, int S, const float* wDown, const float* bDown,
                           const float* wUp, const float* bUp, float slope, float* gate, int N, int C, int R, int H, int W, void* stream);
int isrShuffleTailColourSupported(int N, int C, int Cout, int h, int w, long long fPlane, long long fImage, long long outPlane, long long outImage);
int isrShuffleTailColour(const float* f, long long fPlane, long long fImage, const float* weight, const float* bias, float* out,
                         long long outPlane, long long outImage, int N, int C, int Cout, int h, int w, int clamp, void* stream);

/* Their backward (same tensors, strides, limits and return codes; every sum in a fixed order, no floating-point atomics, no host
 * synchronisation: the launches can be captured in a graph).
 *
 * Channel attention, given dy (dx IS dy: no entry point), the mean z and the gate s [N][64] of the forward (isrChannelPoolMean, `gate`):
 *   isrChannelGateGradSums: workspace[n][c][s] (double, S as above) = the slab sums of dy * t, each product rounded to fp32 once; their sum
 *     in index order, rounded to fp32, is ds[n][c].
 *   isrChannelGateScaleBackward: every workgroup forms ds[64] of its image, du = ds * (s * (1 - s)), recomputes a and g from z as the forward
 *     does, dg[j] = the fp64 sum over c of Wu[c][j] du[c] rounded to fp32, da = a > 0 ? dg : dg * slope, dz[c] = fmaf-chain over j of Wd[j][c] da[j]
 *     from 0, and stores dt = dy * s + (float)(dz[c] / (H W)) as a separately rounded multiply and add.
 *   isrChannelGateParamGrad: one workgroup; dWUp [64][4] = sum_n du g^T, dBUp [64] = sum_n du, dWDown [4][64] = sum_n da z^T,
 *     dBDown [4] = sum_n da, each an fp64 sum over the images in index order, rounded to fp32 once.
 * The tail, given dout [N][Cout][4h][4w]:
 *   isrShuffleTailDataGrad: ONE launch; df[16 ci + 4 i + j][y][x] = dP[ci][4 y + i][4 x + j], dP an fp32 fmaf chain from 0 over (co, ky, kx)
 *     in this nesting of w[co][ci][2 - ky][2 - kx] dout[co][Y + ky - 1][X + kx - 1] (zeros outside the image); the dout tile and its halo
 *     are staged in LDS, the four-channel high-resolution gradient never exists in memory.
 *   isrShuffleTailWeightGrad: TWO launches; per tile (tiles = isrShuffleTailGradTiles(N, h, w)) and output channel the 36 terms of
 *     dw[co][ci][ky][kx] = sum dout[co][Y][X] P[ci][Y + ky - 1][X + kx - 1] and db[co] = sum dout[co] in fp64 -> workspace
 *     double [tiles][Cout][37], then the tiles in index order and one rounding to fp32.  dBias may be NULL. */
int isrChannelAttentionBackwardSupported(int N, int C, int R, int H, int W, long long plane, long long image);      /* each of dy, t, dt */
int isrChannelGateGradSums(const float* dy, long long dyPlane, long long dyImage, const float* t, long long tPlane, long long tImage,
                           int N, int C, int H, int W, int S, double* workspace, void* stream);
int isrChannelGateScaleBackward(const float* dy, long long dyPlane, long long dyImage, float* dt, long long dtPlane, long long dtImage,
                                const double* workspace, int S, const float* mean, const float* gate, const float* wDown, const float* bDown,
                                const float* wUp, float slope, int N, int C, int R, int H, int W, void* stream);
int isrChannelGateParamGrad(const double* workspace, int S, const float* mean, const float* gate, const float* wDown, const float* bDown,
                            const float* wUp, float slope, float* dWDown, float* dBDown, float* dWUp, float* dBUp, int N, int C, int R,
                            int H, int W, void* stream);
int isrShuffleTailBackwardSupported(int N, int C, int Cout, int h, int w, long long fPlane, long long fImage, long long outPlane, long long outImage);
int isrShuffleTailGradTiles(int N, int h, int w);
int isrShuffleTailDataGrad(const float* dout, long long doutPlane, long long doutImage, const float* weight, float* df, long long dfPlane,
                           long long dfImage, int N, int C, int Cout, int h, int w, void* stream);
int isrShuffleTailWeightGrad(const float* dout, long long doutPlane, long long doutImage, const float* f, long long fPlane, long long fImage,
                             int N, int C, int Cout, int h, int w, int tiles, double* workspace, float* dWeight, float* dBias, void* stream);

/* Training-mode batch normalisation of the EnhanceNet blocks (csrc/sr_batchnorm.hip; an eval-mode layer is folded into its convolution
 * on the host side and launches nothing).  x, y, dy, dx, residual: fp32 [N][C][H][W], packed; M = N H W >= 2 values per channel, any
 * C, H, W >= 1, N and C <= 65535 (isrBatchNormSupported says so beforehand: anything else returns -3).  Returns as above.  16-byte
 * accesses where every base address is a multiple of 16 bytes and H W a multiple of four, a per-element path otherwise.  Every sum is
 * taken in fp64 in a fixed order, without floating-point atomics and without host synchronisation: a result depends on the shape only,
 * and the launches can be captured in a graph.
 *   isrBatchNormStats: TWO launches.  Slab sums of x - k and (x - k)^2 (k: the channel's first value) -> workspace
 *     double [C][N S][2], S = isrBatchNormSlabs(N, C, H, W) slabs per plane; then one thread per channel: the partials in index order,
 *     mean[c], invstd[c] = 1 / sqrt(var + eps) with the BIASED variance, both rounded to fp32 once, and -- where the pointers are not
 *     NULL -- running = (1 - momentum) running + momentum {mean, var M / (M - 1)} in place, exactly once per call.
 *   isrBatchNormApply: ONE launch.  y = ((x - mean) * invstd) * gamma + beta with every operation rounded separately, then ReLU (`relu`)
 *     and / or + residual (NULL: none).
 *   isrBatchNormGradSums: TWO launches.  With g = dy where y > 0 and 0 elsewhere (y: the output of the ReLU form; NULL: g = dy) and
 *     xhat = (x - mean) * invstd: slab sums of g and g xhat -> workspace (as above), then dBeta[c] = sum g, dGamma[c] = sum g xhat (either
 *     may be NULL) and coef[c] = {sum g / M, sum g xhat / M} as fp32.
 *   isrBatchNormBackward: ONE launch.  dx = ((g - coef[c][0]) - xhat * coef[c][1]) * (gamma * invstd).  (The gradient of the residual
 *     IS dy: no entry point.) */
int isrBatchNormSupported(int N, int C, int H, int W);
int isrBatchNormSlabs(int N, int C, int H, int W);
int isrBatchNormStats(const float* x, int N, int C, int H, int W, int S, double* workspace, double eps, double momentum, float* mean,
                      float* invstd, float* runningMean, float* runningVar, void* stream);
int isrBatchNormApply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* residual,
                      int relu, float* y, int N, int C, int H, int W, void* stream);
int isrBatchNormGradSums(const float* dy, const float* x, const float* y, const float* mean, const float* invstd, int N, int C, int H, int W,
                         int S, double* workspace, float* coef, float* dGamma, float* dBeta, void* stream);
int isrBatchNormBackward(const float* dy, const float* x, const float* y, const float* mean, const float* invstd, const float* gamma,
                         const float* coef, float* dx, int N, int C, int H, int W, void* stream);

/* Training batches from device-resident clips (csrc/sr_dataset.hip; dataset_video.DeviceClips).  ONE launch on `stream` writes the three
 * packed fp32 tensors of a batch: input [B][T][Cl][c][c], flowOut [B][T][2][c][c], target [B][T][Ch][r c][r c] -- what
 * DatasetFromSamples.__getitem__, data_augmentation and the default collate produce on the host, bit for bit (a value is copied, or
 * copied with its sign bit flipped).
 *   high, low, flow : flat fp32 device buffers holding every clip, [T][Ch][r H][r W], [T][Cl][H][W] and [T][2][H][W], one after the other
 *   clipTable       : device int64 [clips][5]: element offset of the clip in high, in low and in flow, low-resolution height H, width W
 *   sampleTable     : device int32 [numSamples][4]: clip, first row x0 and first column y0 of the low-resolution crop
 *                     [x0, x0 + c) x [y0, y0 + c) (the high-resolution one is r times that), augmentation mode 0..3
 *   indices         : device int64 [B]: the samples of the batch.  The kernel clamps each to [0, numSamples - 1]; the tables are the
 *                     caller's responsibility (offsets inside the buffers, boxes inside their clips).
 *   augment         : 0: no flips.  Otherwise mode bit 0 reverses the rows of all three crops and negates the channels whose bit is set
 *                     in lowNegX / flowNegX, bit 1 reverses the columns and negates the channels of lowNegY / flowNegY.
 *   highQuadAligned : the caller's word that every high offset of clipTable is a multiple of four elements.  With it, r a multiple of
 *                     four and 16-byte aligned `high` and `target`, the high-resolution part moves 16 bytes per lane.
 * All addressing is in 64-bit element offsets.  B <= 65535, Cl and Ch <= 32, fewer than 2^31 values per batch element and tensor
 * (isrClipGatherSupported says so beforehand: anything else returns -3).  No host synchronisation: the launch can be captured. */
int isrClipGatherSupported(int B, int T, int Cl, int Ch, int c, int r);
int isrClipGather(const float* high, const float* low, const float* flow, const long long* clipTable, const int* sampleTable,
                  long long numSamples, const long long* indices, int B, int T, int Cl, int Ch, int c, int r, int augment,
                  unsigned lowNegX, unsigned lowNegY, unsigned flowNegX, unsigned flowNegY, int highQuadAligned,
                  float* input, float* flowOut, float* target, void* stream);

/* The clip generator's frame packer (csrc/sr_dataset.hip: clip_pack_kernel; datagen.py).  ONE launch on `stream` writes one frame of a
 * training clip into the flat clip buffers above, from what the ray-marcher and the flow fill left on the device:
 *   lowGbuffer  [h][w][12], highGbuffer [r h][r w][12] : the two renders of the frame, pixel-interleaved, 16-byte aligned
 *   flow        [2][h][w]                              : the hole-filled flow of the low render (isrFlowFill)
 *   highBuf + highOffset <- six planes [r h][r w]: clamp(g[3], 0, 1) 2 - 1, g[4], g[5], g[6], g[7], g[10]   (mask, normal, depth, AO)
 *   lowBuf  + lowOffset  <- five planes [h][w]   : clamp(g[3], 0, 1) 2 - 1, g[4], g[5], g[6], g[7]
 *   flowBuf + flowOffset <- two planes [h][w]    : copied
 * i.e. convertToNumpy of the reference's DataGenerator/DataGeneratorVideo2.py:66-77 without the files; only the alpha is clamped, as
 * numpy's clip does it (a NaN stays a NaN); every other value keeps its bits.  The offsets are 64-bit element counts; that the frame
 * fits behind them is the caller's responsibility.  With w a multiple of four and 16-byte aligned destinations and flow, planes are
 * written 16 bytes per lane, otherwise float by float: the same values.  r <= 64 and at most 2^26 pixels in the high image
 * (isrClipPackFrameSupported says so beforehand; anything else, or a misaligned G-buffer, returns -3).  No host synchronisation. */
int isrClipPackFrameSupported(int h, int w, int r);
int isrClipPackFrame(const float* lowGbuffer, const float* highGbuffer, const float* flow, int h, int w, int r, float* highBuf,
                     long long highOffset, float* lowBuf, long long lowOffset, float* flowBuf, long long flowOffset, void* stream);

/* Crop coverage of device-resident clips (csrc/sr_dataset.hip: clip_coverage_kernel).  ONE launch, one workgroup per (clip, frame 0 /
 * frame T - 1): tables + tableOffsets[clip] <- int32 [2][H + 1][W + 1], the summed-area tables of the indicator
 * (low[0] + low[1]) + low[2] > 0 (fp32, that order) of the clip's first and last low-resolution frame: entry [y][x] counts the covered
 * pixels of rows < y and columns < x.  low, clipTable: as for isrClipGather ([T][Cl][H][W] per clip, Cl >= 3); tableOffsets: device
 * int64 [numClips], element offsets into `tables`.  Anything else returns -3 (isrClipCoverageSupported). */
int isrClipCoverageSupported(int numClips, int T, int Cl);
int isrClipCoverage(const float* low, const long long* clipTable, const long long* tableOffsets, int numClips, int T, int Cl, int* tables,
                    void* stream);

/* Optional per-dispatch timing of isrConv3x3Forward for benchmarks: while enabled, every forward
 * dispatch carries a start/stop event pair on its own packet (no extra stream operations).
 * isrProfileEnable(1) clears the records and starts recording, (0) stops; (2) also records the frame's small kernels
 * (input assembly, trunk input packing, flow fill, tail finishing: variants 25-30 and the colour networks' 34-36, zero flops).  After synchronising the
 * stream, record i gives variant = 2*MT + upsample (MT = 1|2 M tiles of 32 output channels), the
 * algorithmic FLOPs 2*9*Cin*Cout*N*H*W of the dispatch and its duration in ms. */
int isrProfileEnable(int on);
int isrProfileCount(void);
int isrProfileGet(int i, int* variant, double* flops, float* ms);

#ifdef __cplusplus
}
#endif
#endif
