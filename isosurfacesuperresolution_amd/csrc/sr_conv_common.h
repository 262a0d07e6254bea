// What the fp32 convolution files (sr_conv3x3.hip, sr_wgrad.hip, sr_conv_small.hip) share on the device side.  The operand types, the
// buffer descriptor type, BAD_OFFSET and buf_load are the split-operand kernels' (sr_split_common.h); this adds the workgroup size and
// the tile order.  Everything is inline / static: nothing is called across translation units.
#pragma once
#include "sr_split_common.h"

#ifdef ISR_DIAG
extern int g_conv_dbg;          // isrDebugSetAblation (sr_conv3x3.hip): ablation bits of the fp32 forward and the weight-gradient kernels
#endif

namespace {

constexpr int NTHREADS = 256;

__device__ __forceinline__ int xcd_remap(int bid, int nwg)
{
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

} // namespace
