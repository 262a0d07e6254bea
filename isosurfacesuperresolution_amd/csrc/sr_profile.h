// Per-dispatch timing shared by the translation units of libisr_sr.so (bench.py reads it through isrProfile*; implemented in sr_profile.hip):
// while profiling is enabled, a launcher asks for a start/stop event pair that rides on its dispatch packet
// and registers the launch's kernel variant and algorithmic flops.  Also the host-side helpers every launcher shares: the launch
// itself, the CU count, the LDS opt-in.
#pragma once
#include <hip/hip_runtime.h>

constexpr int ISR_VARIANT_SPLIT = 13;       // conv3x3_split_kernel<false>
constexpr int ISR_VARIANT_SPLIT_UPS = 14;   // conv3x3_split_kernel<true>
constexpr int ISR_VARIANT_SPLIT_STREAM = 15;   // conv3x3_split_stream_kernel
constexpr int ISR_VARIANT_SPLIT_WIDE = 16;     // conv3x3_split_wide_kernel
constexpr int ISR_VARIANT_SPLIT_ROWS2 = 17;    // conv3x3_split_rows2_kernel
constexpr int ISR_VARIANT_SPLIT_TAIL = 18;     // conv3x3_split_tail_kernel (sr_conv_tail.hip)
constexpr int ISR_VARIANT_SPLIT_BLOCK = 19;    // resblock_split_kernel (sr_conv_block.hip)
constexpr int ISR_VARIANT_SPLIT_TRUNK = 20;    // trunk_dataflow_kernel (sr_conv_trunk.hip)
constexpr int ISR_VARIANT_SPLIT_UPS3 = 21;     // conv3x3_split_ups3_kernel (sr_conv_ups3.h)
constexpr int ISR_VARIANT_SPLIT_BLOCK2 = 22;   // conv3x3_split_block2_kernel (sr_conv_block2.h)
constexpr int ISR_VARIANT_SPLIT_UPS4 = 23;     // conv3x3_split_ups4_kernel (sr_conv_ups4.h)
constexpr int ISR_VARIANT_SPLIT_TRUNK_MT = 24; // trunk_mt_kernel (sr_conv_trunk.hip)
// the frame's small kernels (no matrix work: flops = 0); registered so that bench.py can say how much of a frame is BETWEEN kernels
constexpr int ISR_VARIANT_TRUNK_PACK = 25;     // trunk_pack_input_kernel (sr_conv_trunk.hip)
constexpr int ISR_VARIANT_ASSEMBLE = 26;       // assemble_input_kernel (sr_frame.hip)
constexpr int ISR_VARIANT_TAIL_FINISH = 27;    // tail_s_finish_kernel / tail_seam_finish_kernel / tail_combine_finish_kernel (sr_conv_tail.hip)
constexpr int ISR_VARIANT_FLOW_FILL = 28;      // flow_fill_one_kernel / flow_fill_kernel (sr_frame.hip; the frame pipeline runs it on the render stream)
constexpr int ISR_VARIANT_FINISH = 29;         // finish_frame_kernel (sr_frame.hip)
constexpr int ISR_VARIANT_UPS_FRAME = 30;      // ups_frame_kernel (sr_conv_upsp.h): the one-pixel frame of a phase-decomposed upsampling layer
constexpr int ISR_VARIANT_WGRAD_SPLIT = 32;    // conv3x3_wgrad_split2_kernel / conv3x3_wgrad_split_kernel (sr_wgrad.hip): the split-operand weight gradient of one 64 x 64 channel block
constexpr int ISR_VARIANT_SPLIT_UPSP = 31;     // conv3x3_split_upsp_kernel (sr_conv_upsp.h); NOT a "small" kernel: recorded at level 1
// the colour networks' frame kernels (inference/loadedmodel.py, the colour branch)
constexpr int ISR_VARIANT_SPLIT_TAIL_COLOUR = 33;  // conv3x3_split_tail_kernel<2, ., 3> (sr_conv_tail.hip): recorded at level 1, like the six-channel tail
constexpr int ISR_VARIANT_TAIL_FINISH_COLOUR = 34; // tail_s_finish_kernel<3> (sr_conv_tail.hip)             -- small kernels from here on
constexpr int ISR_VARIANT_ASSEMBLE_COLOUR = 35;    // assemble_input_colour_kernel (sr_frame.hip)
constexpr int ISR_VARIANT_FINISH_COLOUR = 36;      // finish_frame_colour_kernel (sr_frame.hip)
// the frame's small kernels are recorded at profiling level 2 only (isrProfileEnable)
constexpr bool isr_variant_is_small(int v) { return (v >= ISR_VARIANT_TRUNK_PACK && v <= ISR_VARIANT_UPS_FRAME) || (v >= ISR_VARIANT_TAIL_FINISH_COLOUR && v <= ISR_VARIANT_FINISH_COLOUR); }

// Sets *e0 / *e1 to an event pair (and records the launch) when profiling is on, leaves them untouched otherwise.
void isr_profile_record(int variant, double flops, hipEvent_t* e0, hipEvent_t* e1);

// THE launch of this library.  While profiling is on the event pair rides on the dispatch packet (hipExtLaunchKernelGGL); otherwise
// the launch is a plain hipLaunchKernelGGL -- the only kind a stream capture (hipGraph) can be relied on to record, so a launch
// without events must never take the Ext path.  Returns 0, or -2 when the runtime refused the launch.
template <typename... Params, typename... Args>
static inline int isr_launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t e0, hipEvent_t e1, const Args&... args)
{
    if (e0 || e1) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, e0, e1, 0, static_cast<Params>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ... of a launch that registers itself as `variant` with `flops` algorithmic flops (0 for the kernels without matrix work)
template <typename... Params, typename... Args>
static inline int isr_launch(int variant, double flops, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args&... args)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    isr_profile_record(variant, flops, &e0, &e1);
    return isr_launch(kernel, grid, block, lds, stream, e0, e1, args...);
}

// Compute units of the current device, looked up once per device ordinal; 256 (an MI355X) where the query fails.
inline int isr_cu_count()
{
    constexpr int MAX_DEVICES = 64;
    static int cus[MAX_DEVICES] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return 256;
    if (!cus[dev] && (hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus[dev] <= 0)) cus[dev] = 256;
    return cus[dev];
}

// "These kernels may use `bytes` of dynamic LDS" (more than 64 KiB needs the opt-in): one hipFuncSetAttribute per kernel per process,
// at the first call of the instantiation, never one per launch.
template <auto... Kernels>
static inline void isr_lds_opt_in(int bytes)
{
    static const bool once = (((void)hipFuncSetAttribute((const void*)Kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)), ..., true);
    (void)once;
}

// Range guard (SplitConvParams::absmax): isrSetRangeFlag(ptr) arms the NEXT launch of a split-operand kernel (any translation
// unit) with a device word that receives the bit pattern of the largest |value| it stores; the launcher takes (and clears) it.
unsigned* isr_take_range_flag();
// Per-wave maxima (SplitConvParams::slotmax): isrSetMaxSlots(words, capacity) arms the NEXT launch of a kernel that supports them (any
// translation unit); the launcher takes (and clears) the array and, if it uses it, says how many words (isrTakeMaxSlotWords reports that).
unsigned* isr_take_max_slots(int* capacity);
void isr_note_max_slot_words(int words);
