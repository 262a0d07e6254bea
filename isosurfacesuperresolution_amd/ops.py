"""Functional bridge between the PyTorch modules and the hand-written HIP kernels.

``conv3x3`` is the one hot op of the super-resolution network (23 of the 24 weight layers and
99.9 % of its FLOPs):

    y = act(conv3x3(U(x), w, padding=1) + bias) + residual         U = optional bilinear x2

* CUDA/HIP tensors: one launch of ``isrConv3x3Forward`` from libisr_sr.so (fp32 MFMA) through the
  C-ABI of ``include/isr_sr_kernels.h``.  Autograd is provided by hand-written kernels as well:
  the data gradient re-uses the forward kernel with flipped/transposed weights, the weight
  gradient is ``isrConv3x3WeightGrad``.  There is no fallback: if the library is missing this raises.
* CPU tensors: the reference's own CPU path, i.e. plain PyTorch ops (BASELINE config #1).
"""
import contextlib
import ctypes
import os
import warnings
import weakref

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _native

ACT_CODES = {'none': 0, 'relu': 1, 'leaky': 2, 'gate': 3}     # 'gate': internal (data gradient through a ReLU)
_lib = None
_warned = set()


def _warn_once(key, message):
    """A device tensor took a PyTorch (MIOpen / ATen) route instead of a kernel of this package: say so, once."""
    if key not in _warned:
        _warned.add(key)
        warnings.warn(message, RuntimeWarning, stacklevel=3)


class _DisplayParams(ctypes.Structure):
    """``IsrDisplayParams`` of include/isr_sr_kernels.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("gbuffer", "rgb", "raw", "flow", "prev", "focus", "focus_mask", "depth_bounds", "out", "out8")] + [
        ("h", ctypes.c_int), ("w", ctypes.c_int), ("channel", ctypes.c_int), ("masking", ctypes.c_int), ("background0", ctypes.c_float),
        ("smooth_prev", ctypes.c_float), ("smooth_cur", ctypes.c_float), ("viewport", ctypes.c_int * 4), ("shading", ctypes.c_float * 18),
        ("exponent", ctypes.c_int), ("ao_strength", ctypes.c_float), ("enable_specular", ctypes.c_int)]


class _DisplayBaselineParams(ctypes.Structure):
    """``IsrDisplayBaselineParams`` of include/isr_sr_kernels.h."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("gbuffer", "low_planes", "flow", "prev", "focus", "focus_mask", "depth_bounds", "out", "out8")] + [
        ("h", ctypes.c_int), ("w", ctypes.c_int), ("mode", ctypes.c_int), ("channel", ctypes.c_int),
        ("smooth_prev", ctypes.c_float), ("smooth_cur", ctypes.c_float), ("viewport", ctypes.c_int * 4), ("shading", ctypes.c_float * 18),
        ("exponent", ctypes.c_int), ("ao_strength", ctypes.c_float), ("enable_specular", ctypes.c_int)]


def _bind(lib):
    """ctypes signatures of include/isr_sr_kernels.h on a loaded build of the library (product or diagnostics: the same ABI)."""
    vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    lib.isrConvCinPad.argtypes = [ci]; lib.isrConvCinPad.restype = ci
    lib.isrConvCoutPad.argtypes = [ci]; lib.isrConvCoutPad.restype = ci
    lib.isrConvPrepareWeights.argtypes = [vp, vp, ci, ci, ci, vp]; lib.isrConvPrepareWeights.restype = ci
    lib.isrConv3x3Forward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ci, vp]
    lib.isrConv3x3Forward.restype = ci
    lib.isrConv3x3ForwardStrided.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ci, ll, ll, ll, ll, ll, ll, vp]
    lib.isrConv3x3ForwardStrided.restype = ci
    lib.isrConvWeightGradWorkspace.argtypes = [ci, ci, ci, ci, ci]; lib.isrConvWeightGradWorkspace.restype = ll
    lib.isrConv3x3WeightGrad.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]; lib.isrConv3x3WeightGrad.restype = ci
    lib.isrConvWeightGradMaxSegments.argtypes = []; lib.isrConvWeightGradMaxSegments.restype = ci
    lib.isrConv3x3WeightGradSegments.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
    lib.isrConv3x3WeightGradSegments.restype = ci
    lib.isrConv3x3WeightGradSegmentsBf16.argtypes = lib.isrConv3x3WeightGradSegments.argtypes
    lib.isrConv3x3WeightGradSegmentsBf16.restype = ci
    lib.isrConv3x3WeightGradSegmentsSplit.argtypes = lib.isrConv3x3WeightGradSegments.argtypes
    lib.isrConv3x3WeightGradSegmentsSplit.restype = ci
    lib.isrActBackward.argtypes = [vp, vp, vp, ll, ci, cf, vp]; lib.isrActBackward.restype = ci
    lib.isrResBlockSmallSupported.argtypes = [ci, ci, ci]; lib.isrResBlockSmallSupported.restype = ci
    lib.isrResBlockSmall.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp]; lib.isrResBlockSmall.restype = ci
    lib.isrConv3x3WeightGradSegmentsSplitMax.argtypes = [vp, vp, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp]
    lib.isrConv3x3WeightGradSegmentsSplitMax.restype = ci
    lib.isrSetMaxSlots.argtypes = [vp, ci]; lib.isrSetMaxSlots.restype = None
    lib.isrTakeMaxSlotWords.argtypes = []; lib.isrTakeMaxSlotWords.restype = ci
    lib.isrAssembleInput.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]; lib.isrAssembleInput.restype = ci
    lib.isrAssembleInputRows.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]; lib.isrAssembleInputRows.restype = ci
    lib.isrAssembleInputRect.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]; lib.isrAssembleInputRect.restype = ci
    lib.isrAssembleInputPacked.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]; lib.isrAssembleInputPacked.restype = ci
    if hasattr(lib, "isrAssembleInputColour"):        # (an older build loaded through ISR_SR_LIB for an A/B run has no colour entry points)
        lib.isrAssembleInputColour.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]; lib.isrAssembleInputColour.restype = ci
        lib.isrFinishFrameColour.argtypes = [vp, vp, vp, ci, ci, vp]; lib.isrFinishFrameColour.restype = ci
        lib.isrConvSmallFinishFrameColour.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ll, vp]; lib.isrConvSmallFinishFrameColour.restype = ci
        lib.isrConvTailWorkspaceBytes3.argtypes = [ci, ci]; lib.isrConvTailWorkspaceBytes3.restype = ll
        lib.isrConvTailPrepare3.argtypes = [vp, vp, vp]; lib.isrConvTailPrepare3.restype = ci
        lib.isrConvTailFinishFrame3.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ll, vp]; lib.isrConvTailFinishFrame3.restype = ci
        lib.isrConvTailFinishFrame3Packed.argtypes = lib.isrConvTailFinishFrame3.argtypes; lib.isrConvTailFinishFrame3Packed.restype = ci
    lib.isrConvSmallCinPad.argtypes = [ci]; lib.isrConvSmallCinPad.restype = ci
    lib.isrConvSmallWeightFloats.argtypes = [ci]; lib.isrConvSmallWeightFloats.restype = ll
    lib.isrConvSmallPrepare.argtypes = [vp, vp, vp, vp, ci, ci, vp]; lib.isrConvSmallPrepare.restype = ci
    lib.isrConv3x3SmallCout.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]; lib.isrConv3x3SmallCout.restype = ci
    lib.isrConv3x3SmallCoutStrided.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ll, ll, vp]
    lib.isrConv3x3SmallCoutStrided.restype = ci
    lib.isrFlowFillWorkspace.argtypes = [ci, ci]; lib.isrFlowFillWorkspace.restype = ll
    lib.isrFlowFill.argtypes = [vp, vp, vp, ci, ci, vp]; lib.isrFlowFill.restype = ci
    lib.isrFlowFillEx.argtypes = [vp, vp, vp, ci, ci, ci, vp]; lib.isrFlowFillEx.restype = ci
    lib.isrFlowFillOne.argtypes = [vp, vp, vp, ci, ci, vp]; lib.isrFlowFillOne.restype = ci
    lib.isrFlowFillOneSupported.argtypes = [ci, ci]; lib.isrFlowFillOneSupported.restype = ci
    lib.isrSetFlowFillErrorWord.argtypes = [vp]; lib.isrSetFlowFillErrorWord.restype = None
    lib.isrFinishFrame.argtypes = [vp, vp, vp, vp, ci, ci, vp, ci, cf, ci, ci, vp]; lib.isrFinishFrame.restype = ci
    lib.isrConvSmallFinishFrame.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ll, vp, ci, cf, ci, ci, vp]
    lib.isrConvSmallFinishFrame.restype = ci
    lib.isrUpsample2xForward.argtypes = [vp, vp, ll, ci, ci, vp]; lib.isrUpsample2xForward.restype = ci
    lib.isrUpsample2xBackward.argtypes = [vp, vp, ll, ci, ci, vp]; lib.isrUpsample2xBackward.restype = ci
    lib.isrReconResidualForward.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]; lib.isrReconResidualForward.restype = ci
    lib.isrReconResidualBackward.argtypes = [vp, vp, ci, ci, ci, ci, ci, ci, vp]; lib.isrReconResidualBackward.restype = ci
    lib.isrLossUnshadedWorkspace.argtypes = []; lib.isrLossUnshadedWorkspace.restype = ll
    lib.isrLossUnshadedForward.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, ctypes.c_uint, vp, cf, ci, vp, vp, vp]
    lib.isrLossUnshadedForward.restype = ci
    lib.isrLossUnshadedBackward.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp, ctypes.c_uint, vp, cf, ci, vp, vp, vp, vp]
    lib.isrLossUnshadedBackward.restype = ci
    if hasattr(lib, "isrLossDownsampleForward"):      # (an older build loaded through ISR_SR_LIB for an A/B run has no ds entry points)
        lib.isrLossDownsampleSupported.argtypes = [ci, ci, ci, ci]; lib.isrLossDownsampleSupported.restype = ci
        lib.isrLossDownsampleWorkspace.argtypes = []; lib.isrLossDownsampleWorkspace.restype = ll
        lib.isrLossDownsampleForward.argtypes = [vp, vp, ci, ci, ci, ci, vp, ctypes.c_uint, vp, cf, ci, vp, vp, vp, vp]
        lib.isrLossDownsampleForward.restype = ci
        lib.isrLossDownsampleBackward.argtypes = [vp, vp, ci, ci, ci, ci, vp, ctypes.c_uint, vp, cf, ci, vp, vp, vp]
        lib.isrLossDownsampleBackward.restype = ci
    lib.isrDiscrInputSupported.argtypes = [ci, ci, ci, ci]; lib.isrDiscrInputSupported.restype = ci
    lib.isrDiscrInputForward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, cf, ci, vp]
    lib.isrDiscrInputForward.restype = ci
    lib.isrDiscrInputBackward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, cf, ci, vp]
    lib.isrDiscrInputBackward.restype = ci
    lib.isrRecurrentInputForward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ll, ll, vp]; lib.isrRecurrentInputForward.restype = ci
    lib.isrRecurrentInputBackward.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ll, vp]; lib.isrRecurrentInputBackward.restype = ci
    lib.isrConvF16WeightBytes.argtypes = [ci, ci]; lib.isrConvF16WeightBytes.restype = ll
    lib.isrConvF16Prepare.argtypes = [vp, vp, ci, ci, vp]; lib.isrConvF16Prepare.restype = ci
    lib.isrConv3x3ForwardF16.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ci, ll, ll, ll, ll, ll, ll, vp]
    lib.isrConvF16SupportsUpsample.argtypes = [ll, ci, ll, ll]; lib.isrConvF16SupportsUpsample.restype = ci
    lib.isrConvBf16Prepare.argtypes = [vp, vp, ci, ci, vp]; lib.isrConvBf16Prepare.restype = ci
    lib.isrConv3x3ForwardBf16.argtypes = lib.isrConv3x3ForwardF16.argtypes; lib.isrConv3x3ForwardBf16.restype = ci
    lib.isrConv3x3ForwardF16.restype = ci
    lib.isrConvSplitWeightBytes.argtypes = [ci, ci]; lib.isrConvSplitWeightBytes.restype = ll
    lib.isrConvSplitPrepare.argtypes = [vp, vp, ci, ci, vp]; lib.isrConvSplitPrepare.restype = ci
    lib.isrConvSplitPrepareManyMax.argtypes = []; lib.isrConvSplitPrepareManyMax.restype = ci
    lib.isrConvSplitPrepareMany.argtypes = [ci, vp, vp, vp, vp, vp, vp]; lib.isrConvSplitPrepareMany.restype = ci
    lib.isrConv3x3ForwardSplit.argtypes = lib.isrConv3x3ForwardF16.argtypes; lib.isrConv3x3ForwardSplit.restype = ci
    lib.isrConvTailWeightBytes.argtypes = []; lib.isrConvTailWeightBytes.restype = ll
    lib.isrConvTailWorkspaceBytes.argtypes = [ci, ci]; lib.isrConvTailWorkspaceBytes.restype = ll
    lib.isrConvTailPrepare.argtypes = [vp, vp, vp]; lib.isrConvTailPrepare.restype = ci
    lib.isrConvTailSupported.argtypes = [vp, ci, ci, ll]; lib.isrConvTailSupported.restype = ci
    lib.isrConvTailFinishFrame.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ll, vp, ci, cf, ci, ci, vp]
    lib.isrConvTailFinishFrame.restype = ci
    lib.isrConv3x3ForwardSplitPacked.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, ci, ll, ll, vp]
    lib.isrConv3x3ForwardSplitPacked.restype = ci
    lib.isrConv3x3ForwardSplitFromPacked.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, ll, ll, ll, vp]
    lib.isrConv3x3ForwardSplitFromPacked.restype = ci
    lib.isrConvTailFinishFramePacked.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ll, vp, ci, cf, ci, ci, vp]
    lib.isrConvTailFinishFramePacked.restype = ci
    lib.isrTrunkDataflowMaxTiles.argtypes = []; lib.isrTrunkDataflowMaxTiles.restype = ci
    lib.isrTrunkDataflowWorkspaceBytes.argtypes = [ci, ci, ci]; lib.isrTrunkDataflowWorkspaceBytes.restype = ll
    lib.isrTrunkDataflowSupported.argtypes = [vp, ci, ci, ci, ll, ll]; lib.isrTrunkDataflowSupported.restype = ci
    lib.isrTrunkDataflow.argtypes = [vp, ci, ll, vp, ll, vp, vp, ci, ci, ci, vp, vp]; lib.isrTrunkDataflow.restype = ci
    lib.isrTrunkDataflowPrepacked.argtypes = [ci, vp, ll, vp, vp, ci, ci, ci, vp, vp]; lib.isrTrunkDataflowPrepacked.restype = ci
    lib.isrTrunkDataflowPackedResult.argtypes = [ci, ci, ci, vp, vp]; lib.isrTrunkDataflowPackedResult.restype = ci
    lib.isrSetTrunkPackedResult.argtypes = [ci]; lib.isrSetTrunkPackedResult.restype = None
    lib.isrConvUpsPhaseWeightBytes.argtypes = []; lib.isrConvUpsPhaseWeightBytes.restype = ll
    lib.isrConvUpsPhaseScratchBytes.argtypes = []; lib.isrConvUpsPhaseScratchBytes.restype = ll
    lib.isrConvUpsPhasePrepare.argtypes = [vp, vp, vp, vp]; lib.isrConvUpsPhasePrepare.restype = ci
    lib.isrConvUpsPhaseSupported.argtypes = [ci, ci, ci, ci, ll, ll]; lib.isrConvUpsPhaseSupported.restype = ci
    lib.isrConvUpsPhase.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, cf, ll, ll, vp]; lib.isrConvUpsPhase.restype = ci
    lib.isrPackSplit.argtypes = [vp, vp, ci, ci, ci, ll, ll, vp]; lib.isrPackSplit.restype = ci
    lib.isrResBlockSplitWorkspaceBytes.argtypes = []; lib.isrResBlockSplitWorkspaceBytes.restype = ll
    lib.isrResBlockSplitSupported.argtypes = [vp, ci, ci, ll, ll]; lib.isrResBlockSplitSupported.restype = ci
    lib.isrResBlockSplit.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, ci, ll, ll, vp]; lib.isrResBlockSplit.restype = ci
    lib.isrAdamFlatStep.argtypes = [vp, vp, vp, vp, ll, vp, cf, ctypes.c_double, ctypes.c_double, cf, vp, vp]; lib.isrAdamFlatStep.restype = ci
    lib.isrSetRangeFlag.argtypes = [vp]; lib.isrSetRangeFlag.restype = None
    lib.isrSetTrunkErrorWord.argtypes = [vp]; lib.isrSetTrunkErrorWord.restype = None
    lib.isrSetTrunkRows.argtypes = [ci]; lib.isrSetTrunkRows.restype = None
    if hasattr(lib, "isrDisplayFrame"):               # (an older build loaded through ISR_SR_LIB for an A/B run has no display stage)
        lib.isrDisplayFrame.argtypes = [ctypes.POINTER(_DisplayParams), vp]; lib.isrDisplayFrame.restype = ci
    if hasattr(lib, "isrDisplayBaselineFrame"):       # (likewise: the render modes came after the display stage)
        lib.isrDisplayBaselineFrame.argtypes = [ctypes.POINTER(_DisplayBaselineParams), vp]; lib.isrDisplayBaselineFrame.restype = ci
    if hasattr(lib, "isrMetricsMsssim"):              # (likewise: the metric stage of the statistics harness, csrc/sr_metrics.hip)
        cd = ctypes.c_double
        lib.isrMetricsSqErr.argtypes = [vp, ll, ll, vp, ll, ll, vp, ll, ci, ci, ci, vp, vp, vp]; lib.isrMetricsSqErr.restype = ci
        lib.isrMetricsMsssimWorkspace.argtypes = [ci, ci, ci]; lib.isrMetricsMsssimWorkspace.restype = ll
        lib.isrMetricsMsssim.argtypes = [vp, ll, ll, vp, ll, ll, vp, ll, ci, ci, ci, vp, vp, vp, vp]; lib.isrMetricsMsssim.restype = ci
        lib.isrMetricsAbsDiffHistogram.argtypes = [vp, ll, ll, vp, ll, ll, vp, ll, ci, ci, ci, cd, ci, vp, vp, vp]
        lib.isrMetricsAbsDiffHistogram.restype = ci
    if hasattr(lib, "isrConvTranspose3x3S2ForwardSplit"):       # (likewise: the transposed convolution, csrc/sr_conv_transpose.hip)
        lib.isrConvTransposeSplitWeightBytes.argtypes = []; lib.isrConvTransposeSplitWeightBytes.restype = ll
        lib.isrConvTransposeSplitPrepare.argtypes = [vp, vp, vp]; lib.isrConvTransposeSplitPrepare.restype = ci
        lib.isrConvTranspose3x3S2SplitSupported.argtypes = [ci, ci, ci, ci, ll, ll]; lib.isrConvTranspose3x3S2SplitSupported.restype = ci
        lib.isrConvTranspose3x3S2ForwardSplit.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, cf, ll, ll, vp]
        lib.isrConvTranspose3x3S2ForwardSplit.restype = ci
    if hasattr(lib, "isrConvTranspose3x3S2DataGradSplit"):      # (likewise: its backward -- phase-major gradient and data gradient)
        lib.isrConvTransposePhaseGradient.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, cf, vp]; lib.isrConvTransposePhaseGradient.restype = ci
        lib.isrConvTranspose3x3S2ForwardSplitBatch.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]
        lib.isrConvTranspose3x3S2ForwardSplitBatch.restype = ci
        lib.isrConvTransposeDataGradWeightBytes.argtypes = []; lib.isrConvTransposeDataGradWeightBytes.restype = ll
        lib.isrConvTransposeDataGradPrepare.argtypes = [vp, vp, vp]; lib.isrConvTransposeDataGradPrepare.restype = ci
        lib.isrConvTranspose3x3S2DataGradSplitSupported.argtypes = [ci, ci, ci, ci]; lib.isrConvTranspose3x3S2DataGradSplitSupported.restype = ci
        lib.isrConvTranspose3x3S2DataGradSplit.argtypes = [vp, vp, vp, ci, ci, ci, ci, vp]; lib.isrConvTranspose3x3S2DataGradSplit.restype = ci
    if hasattr(lib, "isrConv3x3S2Forward"):                     # (likewise: the stride-2 convolution, csrc/sr_conv_stride2.hip)
        lib.isrConv3x3S2Supported.argtypes = [ci, ci, ci, ci, ci]; lib.isrConv3x3S2Supported.restype = ci
        lib.isrConv3x3S2Forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]; lib.isrConv3x3S2Forward.restype = ci
        lib.isrConv3x3S2DataGrad.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, vp]; lib.isrConv3x3S2DataGrad.restype = ci
        lib.isrConv3x3S2WeightGradWorkspace.argtypes = [ci, ci, ci, ci, ci]; lib.isrConv3x3S2WeightGradWorkspace.restype = ll
        lib.isrConv3x3S2WeightGradSegments.argtypes = [vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        lib.isrConv3x3S2WeightGradSegments.restype = ci
    if hasattr(lib, "isrChannelGateScaleAdd"):                  # (likewise: RCAN's channel attention and pixel-shuffle tail, csrc/sr_attention.hip)
        lib.isrChannelPoolSlabs.argtypes = [ci, ci, ci]; lib.isrChannelPoolSlabs.restype = ci
        lib.isrChannelPoolSupported.argtypes = [ci, ci, ci, ci, ll, ll]; lib.isrChannelPoolSupported.restype = ci
        lib.isrChannelGateScaleAddSupported.argtypes = [ci, ci, ci, ci, ci, ll, ll]; lib.isrChannelGateScaleAddSupported.restype = ci
        lib.isrChannelPool.argtypes = [vp, ll, ll, ci, ci, ci, ci, ci, vp, vp]; lib.isrChannelPool.restype = ci
        lib.isrChannelPoolMean.argtypes = [vp, ci, ci, ci, ci, ci, vp, vp]; lib.isrChannelPoolMean.restype = ci
        lib.isrChannelGateScaleAdd.argtypes = [vp, vp, vp, ll, ll, ll, ll, ll, ll, vp, ci, vp, vp, vp, vp, cf, vp, ci, ci, ci, ci, ci, vp]
        lib.isrChannelGateScaleAdd.restype = ci
        lib.isrShuffleTailColourSupported.argtypes = [ci, ci, ci, ci, ci, ll, ll, ll, ll]; lib.isrShuffleTailColourSupported.restype = ci
        lib.isrShuffleTailColour.argtypes = [vp, ll, ll, vp, vp, vp, ll, ll, ci, ci, ci, ci, ci, ci, vp]; lib.isrShuffleTailColour.restype = ci
    if hasattr(lib, "isrChannelGateScaleBackward"):             # (likewise: their backward; without it they train on the torch composite)
        lib.isrChannelAttentionBackwardSupported.argtypes = [ci, ci, ci, ci, ci, ll, ll]; lib.isrChannelAttentionBackwardSupported.restype = ci
        lib.isrChannelGateGradSums.argtypes = [vp, ll, ll, vp, ll, ll, ci, ci, ci, ci, ci, vp, vp]; lib.isrChannelGateGradSums.restype = ci
        lib.isrChannelGateScaleBackward.argtypes = [vp, ll, ll, vp, ll, ll, vp, ci, vp, vp, vp, vp, vp, cf, ci, ci, ci, ci, ci, vp]
        lib.isrChannelGateScaleBackward.restype = ci
        lib.isrChannelGateParamGrad.argtypes = [vp, ci, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        lib.isrChannelGateParamGrad.restype = ci
        lib.isrShuffleTailBackwardSupported.argtypes = [ci, ci, ci, ci, ci, ll, ll, ll, ll]; lib.isrShuffleTailBackwardSupported.restype = ci
        lib.isrShuffleTailGradTiles.argtypes = [ci, ci, ci]; lib.isrShuffleTailGradTiles.restype = ci
        lib.isrShuffleTailDataGrad.argtypes = [vp, ll, ll, vp, vp, ll, ll, ci, ci, ci, ci, ci, vp]; lib.isrShuffleTailDataGrad.restype = ci
        lib.isrShuffleTailWeightGrad.argtypes = [vp, ll, ll, vp, ll, ll, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]; lib.isrShuffleTailWeightGrad.restype = ci
    if hasattr(lib, "isrBatchNormStats"):                       # (likewise: training-mode batch normalisation, csrc/sr_batchnorm.hip)
        cd = ctypes.c_double
        lib.isrBatchNormSupported.argtypes = [ci, ci, ci, ci]; lib.isrBatchNormSupported.restype = ci
        lib.isrBatchNormSlabs.argtypes = [ci, ci, ci, ci]; lib.isrBatchNormSlabs.restype = ci
        lib.isrBatchNormStats.argtypes = [vp, ci, ci, ci, ci, ci, vp, cd, cd, vp, vp, vp, vp, vp]; lib.isrBatchNormStats.restype = ci
        lib.isrBatchNormApply.argtypes = [vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, vp]; lib.isrBatchNormApply.restype = ci
        lib.isrBatchNormGradSums.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]; lib.isrBatchNormGradSums.restype = ci
        lib.isrBatchNormBackward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]; lib.isrBatchNormBackward.restype = ci
    if hasattr(lib, "isrClipGather"):                           # (likewise: training batches from device-resident clips, csrc/sr_dataset.hip)
        cu = ctypes.c_uint
        lib.isrClipGatherSupported.argtypes = [ci, ci, ci, ci, ci, ci]; lib.isrClipGatherSupported.restype = ci
        lib.isrClipGather.argtypes = [vp, vp, vp, vp, vp, ll, vp, ci, ci, ci, ci, ci, ci, ci, cu, cu, cu, cu, ci, vp, vp, vp, vp]
        lib.isrClipGather.restype = ci
    if hasattr(lib, "isrClipPackFrame"):                        # (likewise: the clip generator's frame packer and crop coverage)
        lib.isrClipPackFrameSupported.argtypes = [ci, ci, ci]; lib.isrClipPackFrameSupported.restype = ci
        lib.isrClipPackFrame.argtypes = [vp, vp, vp, ci, ci, ci, vp, ll, vp, ll, vp, ll, vp]; lib.isrClipPackFrame.restype = ci
        lib.isrClipCoverageSupported.argtypes = [ci, ci, ci]; lib.isrClipCoverageSupported.restype = ci
        lib.isrClipCoverage.argtypes = [vp, vp, vp, ci, ci, ci, vp, vp]; lib.isrClipCoverage.restype = ci
    lib.isrProfileEnable.argtypes = [ci]; lib.isrProfileEnable.restype = ci
    lib.isrProfileCount.argtypes = []; lib.isrProfileCount.restype = ci
    lib.isrProfileGet.argtypes = [ci, vp, vp, vp]; lib.isrProfileGet.restype = ci
    if hasattr(lib, "isrDebugSplitState"):            # the diagnostics build (csrc/sr_diag.h): its switches on top
        lib.isrDebugSetFlowFillFault.argtypes = [ci, ctypes.c_ulonglong]; lib.isrDebugSetFlowFillFault.restype = None
        lib.isrDebugSetTrunkFault.argtypes = [ci, ctypes.c_ulonglong]; lib.isrDebugSetTrunkFault.restype = None
        lib.isrDebugSetTrunkMultiTile.argtypes = [ci]; lib.isrDebugSetTrunkMultiTile.restype = None
        for name in ("isrDebugSetSplitAlgo", "isrDebugSetSplitUpsForm", "isrDebugSetSplitSlots", "isrDebugSetSplitSmall", "isrDebugSetSplitAblation",
                     "isrDebugSetTailFused", "isrDebugSetForwardTile", "isrDebugSetForwardAlgo", "isrDebugSetWgradSplitForm", "isrDebugSetAblation",
                     "isrDebugSetTrunkAblation", "isrDebugSetBlockAblation", "isrDebugSetF16Ablation"):
            getattr(lib, name).argtypes = [ci]; getattr(lib, name).restype = None
        for name in ("isrDebugSplitState", "isrDebugTailState", "isrDebugBlockState", "isrDebugTrunkState", "isrDebugFlowFillState",
                     "isrDebugSplitUpsForm", "isrDebugWgradSplitForm"):
            getattr(lib, name).argtypes = []; getattr(lib, name).restype = ci
        for name in ("isrDebugSetSplitStampBuffer", "isrDebugSetTrunkStampBuffer", "isrDebugSetBlockStampBuffer", "isrDebugSetF16StampBuffer",
                     "isrDebugSetStampBuffer"):
            getattr(lib, name).argtypes = [vp]; getattr(lib, name).restype = None
    return lib


def _sr():
    global _lib
    if _lib is None:
        _lib = _bind(_native.load(_native.SR_LIB))
    return _lib


def is_diagnostics_library():
    """Is the library this process launches on the DIAGNOSTICS build (isrDebug* switches, stamp buffers, fault injection, the experimental
    kernel forms)?  The product build -- what a deployment ships and what bench.py / the driver measure -- has none of them."""
    return hasattr(_sr(), "isrDebugSplitState")


@contextlib.contextmanager
def diagnostics_library():
    """Run the enclosed launches on the DIAGNOSTICS build of the kernels (lib/libisr_sr_diag.so, `make diag`), then go back to the product
    build: the tests of the timeout paths (fault injection) and of kernel forms only a switch selects, and tools/.  The two builds are
    the same sources and the same ABI; weight images and workspaces made by one are valid for the other, the per-launch globals (range
    flag, error words, trunk rows) are set by ``ops`` at every launch.  Single-threaded by contract, like the libraries."""
    global _lib
    saved = _sr()
    if hasattr(saved, "isrDebugSplitState"):          # already there (ISR_SR_DIAG=1 / ISR_SR_LIB=...)
        yield saved
        return
    torch.cuda.synchronize()
    diag = _bind(_native.load(_native.SR_DIAG_LIB))
    assert hasattr(diag, "isrDebugSplitState"), "%s is not a diagnostics build (make -C csrc diag)" % _native.SR_DIAG_LIB
    was_profiling = _profile_on
    _lib = diag
    try:
        if was_profiling:
            diag.isrProfileEnable(1)
        yield diag
    finally:
        torch.cuda.synchronize()
        if was_profiling:
            diag.isrProfileEnable(0)
        _lib = saved


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# Inference re-uses the re-laid-out weights for as long as the very same tensor object is alive and
# unmodified (a data_ptr alone is not an identity: the caching allocator recycles addresses).
# ``weight._version`` does not see every change: a HIP-graph replay of a training step (train.GraphedTrainStep) runs the
# captured optimizer kernels on the parameters' memory without touching the Python-side version counter.  Whoever changes
# weights behind autograd's back therefore calls ``invalidate_weight_images()``; every cached image carries the epoch
# it was made in and is rebuilt when the epoch has moved on.
_images_epoch = 0


def invalidate_weight_images():
    """Declare every cached kernel-layout weight image (exact, small-Cout, fp16 / bf16, split) stale."""
    global _images_epoch
    _images_epoch += 1


class _WeightImages:
    """The kernel-layout images of one kernel family: ``key`` (the caller's: id(weight) and the layout flags) -> image, valid while
    the rule above holds for ``tensors`` -- (weight,), or (weight, bias-or-None) where the image holds the bias too."""

    def __init__(self, cap=512):
        self.cap, self.entries = cap, {}

    @staticmethod
    def _stamp(tensors):
        return tuple((t._version, t.data_ptr()) if t is not None else None for t in tensors)

    def lookup(self, key, tensors):
        hit = self.entries.get(key)
        if hit is not None and hit[0]() is tensors[0] and hit[1] == self._stamp(tensors) and hit[3] == _images_epoch:
            return hit[2]
        return None

    def store(self, key, tensors, image):
        # Beyond the cap only entries whose weight is dead go, never a live one: a captured frame (pipeline._frame_graph) or a
        # launch in flight may hold the image's address.
        if len(self.entries) > self.cap:
            for k in [k for k, v in self.entries.items() if v[0]() is None]:
                del self.entries[k]
        self.entries[key] = (weakref.ref(tensors[0]), self._stamp(tensors), image, _images_epoch)

    def get(self, key, tensors, build, what):
        """The cached image, or the one ``build()`` makes now: it returns (image, return code of the library call ``what``)."""
        image = self.lookup(key, tensors)
        if image is None:
            image, rc = build()
            if rc != 0:
                raise RuntimeError("%s failed (%d)" % (what, rc))
            self.store(key, tensors, image)
        return image

    def clear(self):
        self.entries.clear()


_wcache = _WeightImages()


# ---- routing epoch: what a CAPTURED frame (pipeline.SuperResolutionPipeline, ISR_FRAME_GRAPH) has baked in ----------------------
# A captured HIP graph holds raw device pointers and the routing decisions of the moment it was captured: which kernel form ran
# (dataflow trunk or per-layer, one-launch or three-launch flow fill), which guard word a launch reports to, which workspace it
# spins in.  Every code path that changes one of these behind a graph's back moves this epoch (``_trunk_failed``,
# ``_fill_failed``, ``range_reset``, ``set_device_shared``); the pipeline puts it -- with the switches themselves and the weights'
# (version, address) -- into the signature that decides whether its captured frames are still valid.
_routing_epoch = 0


def routing_epoch():
    return _routing_epoch


def _routing_changed():
    global _routing_epoch
    _routing_epoch += 1


# Several processes (or several independent streams of kernels) share ONE device: the all-resident spin kernels -- the dataflow
# trunk (one workgroup per CU, neighbours wait for each other) and the one-launch flow fill (every workgroup waits for the last) --
# assume that all workgroups of a launch are resident at once; beside another process's grid they may not be, and then they wait
# for each other until the 50 ms deadline.  With the hint set those forms are refused everywhere (``trunk_supported``,
# ``fill_flow_gbuffer``) and the per-layer / three-launch forms run: bit-identical results.  ISR_DEVICE_SHARED=1 or
# ``set_device_shared(True)`` (bench.py: BENCH_SHARE_DEVICE=1, in every mode).
DEVICE_SHARED = os.environ.get("ISR_DEVICE_SHARED", "0") == "1"


def set_device_shared(on):
    global DEVICE_SHARED
    on = bool(on)
    if on != DEVICE_SHARED:
        DEVICE_SHARED = on
        _routing_changed()


def spin_kernel_forms():
    """Which of the all-resident forms a launch may take right now (bench lines and tests report it)."""
    return {"trunk_dataflow": bool(TRUNK_DATAFLOW and not DEVICE_SHARED), "flow_fill_one": bool(FLOW_FILL_ONE and not DEVICE_SHARED)}


def prepare_weights(weight, transpose_flip=False):
    """PyTorch [Cout,Cin,3,3] -> kernel layout [9][cinPad][coutPad] (device tensor)."""
    lib = _sr()

    def build():
        cout, cin = weight.shape[0], weight.shape[1]
        rows, k = (cin, cout) if transpose_flip else (cout, cin)
        wp = torch.empty(9 * lib.isrConvCinPad(k) * lib.isrConvCoutPad(rows), dtype=torch.float32, device=weight.device)
        return wp, lib.isrConvPrepareWeights(_ptr(weight.detach().contiguous()), _ptr(wp), cout, cin, 1 if transpose_flip else 0, _stream())
    return _wcache.get((id(weight), bool(transpose_flip)), (weight,), build, "isrConvPrepareWeights")


# Optional per-dispatch timing for bench.py: the library attaches start/stop events to the
# dispatch packets themselves (isrProfile*), which does not add stream operations.
VARIANT_NAMES = {6: "conv3x3_small_cout_kernel", 2: "conv3x3_fwd_kernel<1,false>", 3: "conv3x3_fwd_kernel<1,true>",
                 4: "conv3x3_fwd_kernel<2,false>", 5: "conv3x3_fwd_kernel<2,true>",
                 8: "conv3x3_fwd2_kernel<false,4>", 9: "conv3x3_fwd2_kernel<true,4>",
                 10: "conv3x3_fwd2_kernel<false,1>", 11: "conv3x3_fwd2_kernel<true,1>", 12: "conv3x3_rowsplit_kernel",
                 13: "conv3x3_split_kernel<false>", 14: "conv3x3_split_kernel<true>",
                 15: "conv3x3_split_stream_kernel", 16: "conv3x3_split_wide_kernel", 17: "conv3x3_split_rows2_kernel",
                 18: "conv3x3_split_tail_kernel", 19: "resblock_split_kernel", 20: "trunk_dataflow_kernel",
                 21: "conv3x3_split_ups3_kernel", 22: "conv3x3_split_block2_kernel", 23: "conv3x3_split_ups4_kernel",
                 24: "trunk_mt_kernel",
                 # the frame's small kernels (zero algorithmic flops; registered for bench.py's gap accounting)
                 25: "trunk_pack_input_kernel", 26: "assemble_input_kernel", 27: "tail_finish_kernel", 28: "flow_fill_one_kernel",
                 29: "finish_frame_kernel", 30: "ups_frame_kernel", 31: "conv3x3_split_upsp_kernel",
                 32: "conv3x3_wgrad_split_kernel",
                 # the colour networks' frame kernels (33 carries the tail's matrix work; 34-36 are small kernels)
                 33: "conv3x3_split_tail_colour_kernel", 34: "tail_finish_colour_kernel", 35: "assemble_input_colour_kernel",
                 36: "finish_frame_colour_kernel",
                 # the transposed convolution of the TecoGAN generator (csrc/sr_conv_transpose.hip)
                 37: "convt3x3s2_split_kernel", 38: "convt3x3s2_dgrad_split_kernel",
                 # RCAN's channel attention and pixel-shuffle tail (csrc/sr_attention.hip)
                 39: "channel_pool_kernel", 40: "gate_scale_add_kernel", 41: "shuffle_tail_kernel",
                 # ... and their backward
                 42: "gate_grad_sum_kernel", 43: "gate_backward_kernel", 44: "gate_param_grad_kernel",
                 45: "shuffle_tail_dgrad_kernel", 46: "shuffle_tail_wgrad_kernel", 47: "shuffle_tail_wgrad_sum_kernel",
                 # the stride-2 convolution of the discriminators (csrc/sr_conv_stride2.hip)
                 48: "conv3x3s2_fwd_kernel", 49: "conv3x3s2_dgrad_kernel", 50: "conv3x3s2_wgrad_kernel", 51: "conv3x3s2_wgrad_sum_kernel",
                 # the discriminator inputs of the adversarial terms (csrc/sr_train.hip)
                 52: "discr_input_fwd_kernel", 53: "discr_input_bwd_kernel",
                 # training-mode batch normalisation (csrc/sr_batchnorm.hip): forward 54-56, backward 57-59
                 54: "batch_norm_stat_kernel", 55: "batch_norm_finish_kernel", 56: "batch_norm_apply_kernel",
                 57: "batch_norm_grad_sum_kernel", 58: "batch_norm_grad_finish_kernel", 59: "batch_norm_backward_kernel",
                 # a training batch from device-resident clips (csrc/sr_dataset.hip)
                 60: "clip_gather_kernel",
                 # the clip generator (datagen.py): a rendered frame into the flat clip buffers, crop coverage of the first / last frames
                 61: "clip_pack_kernel", 62: "clip_coverage_kernel"}


def debug_switches():
    """Bit mask of the libraries' process-global diagnostic switches (``isrDebugSet*``: ablations that skip MFMAs, forced kernel
    forms, grid caps, stamp buffers) that are not in their default position; 0 on a clean process.  bench.py reports it and
    refuses to print a headline measured with an ablation active."""
    lib = _sr()
    if not hasattr(lib, "isrDebugSplitState"):        # the product build has no switches (csrc/sr_diag.h): 0 by construction
        return 0
    return (int(lib.isrDebugSplitState()) | (int(lib.isrDebugTailState()) << 8) | (int(lib.isrDebugBlockState()) << 12) | (int(lib.isrDebugTrunkState()) << 16)
            | (int(lib.isrDebugFlowFillState()) << 28))


_profile_on = False


def profile_enable(on, small_kernels=False):
    """``small_kernels``: also the frame's kernels without matrix work (assembly, packing, flow fill, finishing)."""
    global _profile_on
    _profile_on = bool(on)
    _sr().isrProfileEnable((2 if small_kernels else 1) if on else 0)


def profile_is_on():
    """Per-dispatch profiling puts start / stop events on the kernels' dispatch packets: not something to capture into a graph."""
    return _profile_on


def profile_records():
    """[(kernel_name, algorithmic_flops, milliseconds)] of every forward dispatch since profile_enable(True);
    call after synchronising."""
    lib = _sr()
    out = []
    v, f, ms = ctypes.c_int(), ctypes.c_double(), ctypes.c_float()
    for i in range(lib.isrProfileCount()):
        if lib.isrProfileGet(i, ctypes.byref(v), ctypes.byref(f), ctypes.byref(ms)) != 0:
            raise RuntimeError("isrProfileGet failed")
        out.append((VARIANT_NAMES[v.value], f.value, ms.value))
    return out


_small_cache = _WeightImages(64)


def _prepare_small(weight, bias):
    """(w8, bias8) device tensors for the Cout <= 8 kernel, cached like prepare_weights."""
    lib = _sr()

    def build():
        cout, cin = weight.shape[0], weight.shape[1]
        w8 = torch.empty(lib.isrConvSmallWeightFloats(cin), dtype=torch.float32, device=weight.device)
        b8 = torch.empty(8, dtype=torch.float32, device=weight.device)
        return (w8, b8), lib.isrConvSmallPrepare(_ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous()) if bias is not None else None,
                                                 _ptr(w8), _ptr(b8), cout, cin, _stream())
    return _small_cache.get(id(weight), (weight, bias), build, "isrConvSmallPrepare")


def _launch_small(x, weight, bias, residual, act, slope):
    lib = _sr()
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    w8, b8 = _prepare_small(weight, bias)
    x, xp, xi = _plane_strides(x)
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device)
    rc = lib.isrConv3x3SmallCoutStrided(_ptr(x), _ptr(w8), _ptr(b8), _ptr(residual), _ptr(y), n, cin, h, w, cout,
                                        ACT_CODES[act], float(slope), xp, xi, _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3SmallCout failed (%d)" % rc)
    return y


# Channel-plane padding of large activations.  A [64][1080][1920] fp32 tensor has planes of exactly
# 2025 x 4 KiB; when the 1080p conv reads 64 such planes and writes 64 more (same rows of every plane at the
# same time) the accesses alias in the memory system and the layer drops from 125 to 105 TFLOP/s
# (tools/lab/bench_conv_pad.py: any padding >= 16 floats on BOTH tensors cures it, padding one of them does not).
# Activations the conv kernels allocate themselves therefore get one extra row between channel planes once a
# plane reaches PLANE_PAD_MIN_BYTES; every consumer in this package takes the strides from the tensor
# (`_plane_strides`), anything else sees an ordinary strided view.
PLANE_PAD_MIN_BYTES = 4 << 20
PLANE_PAD_ROWS = 1


def plane_pad(h, w):
    return PLANE_PAD_ROWS * ((w + 3) // 4) * 4 if h * w * 4 >= PLANE_PAD_MIN_BYTES else 0


def empty_planes(n, c, h, w, device):
    """[n, c, h, w] fp32 tensor with packed rows and (possibly) padded channel planes."""
    plane = h * w + plane_pad(h, w)
    if plane == h * w:
        return torch.empty((n, c, h, w), dtype=torch.float32, device=device)
    return torch.empty(n * c * plane, dtype=torch.float32, device=device).as_strided((n, c, h, w), (c * plane, plane, w, 1))


def _plane_strides(t):
    """(tensor, plane stride, image stride) with packed rows; copies only if the rows are not packed."""
    n, c, h, w = t.shape
    if t.stride(3) == 1 and t.stride(2) == w and t.stride(1) >= h * w and (n == 1 or t.stride(0) >= c * t.stride(1)):
        return t, t.stride(1), t.stride(0) if n > 1 else c * t.stride(1)
    t = t.contiguous()
    return t, h * w, c * h * w


def _launch_forward(x, wprep, bias, residual, cin, cout, act, slope, upsample2x, packed=False):
    """``packed``: the result is an ordinary contiguous tensor (the autograd paths hand raw pointers of saved outputs
    to kernels that index them flat); otherwise large channel planes are padded (``empty_planes``)."""
    lib = _sr()
    n, _, hin, win = x.shape
    h, w = (hin * 2, win * 2) if upsample2x else (hin, win)
    x, xp, xi = _plane_strides(x)
    rp = ri = 0
    if residual is not None:
        residual, rp, ri = _plane_strides(residual)
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device) if packed else empty_planes(n, cout, h, w, x.device)
    rc = lib.isrConv3x3ForwardStrided(_ptr(x), _ptr(wprep), _ptr(bias), _ptr(residual), _ptr(y),
                                      n, cin, h, w, cout, ACT_CODES[act], float(slope), 1 if upsample2x else 0,
                                      xp, xi, y.stride(1), cout * y.stride(1), rp, ri, _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3ForwardStrided failed (%d)" % rc)
    return y


# ---- fp16 fast mode (inference only, NOT the parity path) ------------------------------------------------------
# FAST_F16 = True routes the no-grad ``conv3x3`` of layers with more than 8 output channels through
# ``isrConv3x3ForwardF16`` (operands rounded to fp16, fp32 accumulation, fp32 tensors).  Off by default: the 1e-4
# parity with the reference's CPU path is a property of the fp32 kernels.  bench.py reports it separately with its PSNR.
FAST_F16 = False
_f16_cache = _WeightImages()


def _prepare_lp(weight, transpose_flip=False, bf16=False):
    """Weights in the low-precision kernel's layout (fp16, or bf16 for the training mode); transpose_flip: the
    data-gradient weights w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]."""
    lib = _sr()

    def build():
        w = weight.detach()
        if transpose_flip:
            w = w.flip(2, 3).transpose(0, 1)
        w = w.contiguous()
        cout, cin = w.shape[0], w.shape[1]
        wq = torch.empty(lib.isrConvF16WeightBytes(cin, cout), dtype=torch.uint8, device=weight.device)
        return wq, (lib.isrConvBf16Prepare if bf16 else lib.isrConvF16Prepare)(_ptr(w), _ptr(wq), cout, cin, _stream())
    return _f16_cache.get((id(weight), bool(transpose_flip), bool(bf16)), (weight,), build, "isrConv%sPrepare" % ("Bf16" if bf16 else "F16"))


def _launch_lp(symbol, x, wq, bias, residual, cout, act, slope, upsample2x, packed=False):
    """One launch of the library's ``symbol`` = "isrConv3x3ForwardF16" / "...Bf16" / "...Split", which share one signature (x: fp32
    NCHW, channel planes may be padded; ``packed`` as in ``_launch_forward``)."""
    lib = _sr()
    x, xp, xi = _plane_strides(x)
    fuse = False
    if upsample2x:
        fuse = bool(lib.isrConvF16SupportsUpsample(x.data_ptr(), x.shape[3], xp, xi))
        if not fuse:          # unaligned low-res rows: the resize runs as its own kernel first
            x, xp, xi = _plane_strides(bilinear_upsample2x(x))
    n, cin = x.shape[0], x.shape[1]
    h, w = (2 * x.shape[2], 2 * x.shape[3]) if fuse else (x.shape[2], x.shape[3])
    rp = ri = 0
    if residual is not None:
        residual, rp, ri = _plane_strides(residual)
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x.device) if packed else empty_planes(n, cout, h, w, x.device)
    rc = getattr(lib, symbol)(_ptr(x), _ptr(wq), _ptr(bias), _ptr(residual), _ptr(y), n, cin, h, w, cout, ACT_CODES[act], float(slope),
                              1 if fuse else 0, xp, xi, y.stride(1), cout * y.stride(1), rp, ri, _stream())
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (symbol, rc))
    return y


def conv3x3_f16(x, weight, bias=None, act='none', slope=0.01, residual=None, upsample2x=False):
    """``conv3x3`` in the fp16 fast mode (no autograd): y = act(conv3x3(U(x), fp16(w)) + bias) + residual."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    with torch.no_grad():
        return _launch_lp("isrConv3x3ForwardF16", x, _prepare_lp(weight), bias.contiguous() if bias is not None else None, residual,
                          weight.shape[0], act, slope, upsample2x)


# ---- range guard of the split-operand path, and the per-frame guard words ---------------------------------------------------
# The split of an ACTIVATION into (hi, lo') fp16 numbers overflows at |x| >= 65520 (inf / NaN downstream: loud, not silent).  With
# the reference's networks and G-buffer inputs in [-1, 5] this cannot happen; a user's checkpoint is one badly scaled layer away
# (inference/loadedmodel.py:70-120 of the reference: arbitrary checkpoints, arbitrary sequences).  So every split-operand launch
# leaves the largest |value| it stored in a device word (SplitConvParams::absmax, one atomic per wave) and tensors remember which
# word describes them.  Producers whose output came within a factor two of the limit are HOT: the CONSUMER of a hot tensor (and,
# conservatively, everything downstream of it in that frame) runs on the exact fp32 kernels (sr_conv3x3.hip), which have the full
# fp32 range.  Two ways the host learns about it, neither a synchronisation inside a frame:
#   * a model's FIRST frame: ``range_check_due`` -> ``refresh_range_flags`` reads the words (one synchronisation) and the frame is
#     computed again with the routing -- repeated, because a fused launch only says THAT something inside it was hot and the
#     per-layer pass that replaces it says where: the first frame of any checkpoint is right;
#   * EVERY later frame, one frame late (``guards_publish`` / ``guards_poll``): the frame ends with an asynchronous copy of the
#     words into pinned host memory, the next frame starts by reading that copy -- a plain load.  A layer that turns hot at frame t
#     is routed from frame t + 1 on (a fused segment is then taken apart conservatively: all its layers count as hot).  The
#     threshold (3e4) is a factor two below the overflow, so values that GROW into the limit are caught while they are still exact.
# The last word of the buffer is the dataflow trunk's error word (``isrSetTrunkErrorWord``): a launch that gave up waiting for a
# neighbour raises at the start of the NEXT frame and switches the dataflow form off for the process.
RANGE_GUARD = True
RANGE_LIMIT = 3.0e4
_RANGE_SLOTS = 512
_TRUNK_ERROR_SLOT = _RANGE_SLOTS - 1
_FILL_ERROR_SLOT = _RANGE_SLOTS - 2       # ... and the word before it the one-launch flow fill's (``isrSetFlowFillErrorWord``), same rule
HOT = "hot"                      # range key of a tensor of unknown / large range (e.g. produced by an exact kernel on the guarded path)
_range = {}                      # device -> state, see _range_state


def _range_state(device):
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    st = _range.get(device)
    if st is None:
        st = {"buf": torch.zeros(_RANGE_SLOTS, dtype=torch.int32, device=device), "slots": {}, "hot": set(), "frames": 0,
              "members": {},                # fused segment key -> keys of the layers it covers
              "mirror": torch.zeros(_RANGE_SLOTS, dtype=torch.int32).pin_memory(), "event": torch.cuda.Event(), "pending": False}
        _range[device] = st
    return st


def _arm_range(key, device, members=None):
    """Arm the NEXT split-operand launch with the flag word of producer ``key`` (no-op when the guard is off).  ``members``: the
    per-layer keys a fused launch stands for.  Out of words: the tensor counts as HOT (its consumer takes the exact kernel) -- an
    unguarded launch is never silently accepted."""
    if not RANGE_GUARD:
        return None
    st = _range_state(device)
    idx = st["slots"].get(key)
    if idx is None:
        if len(st["slots"]) >= _FILL_ERROR_SLOT:
            _warn_once("range_slots", "range guard: all %d flag words are in use (models loaded without ops.range_reset()?); "
                       "further layers' consumers run on the exact fp32 kernels" % _FILL_ERROR_SLOT)
            return HOT
        idx = st["slots"][key] = len(st["slots"])
    if members is not None:
        st["members"][key] = tuple(members)
    _sr().isrSetRangeFlag(ctypes.c_void_p(st["buf"].data_ptr() + 4 * idx))
    return key


def range_is_hot(key, device):
    """Must a consumer of the tensor tagged ``key`` avoid the split kernels?"""
    if key is None or not RANGE_GUARD:
        return False
    return key == HOT or key in _range_state(device)["hot"]


def any_hot(device):
    if not RANGE_GUARD:
        return False
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    return device in _range and bool(_range[device]["hot"])


def _mark_hot(st, words, conservative):
    """``words``: the guard words as a float32 view (host).  -> the producers that became hot.  ``conservative``: a fused segment
    that is hot makes every layer it covers hot at once (nobody recomputes the frame to find out which one it was)."""
    new = set()
    n = len(st["slots"])
    words = words.numpy() if torch.is_tensor(words) else words
    if n == 0 or bool((words[:n] < RANGE_LIMIT).all()):              # the common case in one vector compare (slots are handed out 0, 1, 2, ...)
        return new
    for key, idx in st["slots"].items():
        v = float(words[idx])
        if not (v < RANGE_LIMIT) and key not in st["hot"]:           # NaN compares false: hot
            st["hot"].add(key)
            new.add(key)
            if conservative:
                for m in st["members"].get(key, ()):
                    if m not in st["hot"]:
                        st["hot"].add(m)
                        new.add(m)
    return new


def refresh_range_flags(device=None):
    """Read the producers' maxima (ONE host synchronisation), mark producers at or above RANGE_LIMIT (or non-finite) hot (the
    words are running maxima and stay: hot is a one-way state until ``range_reset``).  Returns the set of producers that became hot in this call.  (Also a moment the dataflow trunk's error
    word is looked at, ``trunk_check``.)"""
    trunk_check()
    new = set()
    for dev, st in list(_range.items()):
        if device is not None and dev != _range_device(device):
            continue
        if not st["slots"]:
            continue
        vals = st["buf"].cpu().view(torch.float32)
        new |= _mark_hot(st, vals, conservative=False)
        st["pending"] = False
    return new


def _range_device(device):
    device = torch.device(device)
    return device if device.index is not None else torch.device(device.type, torch.cuda.current_device())


def guards_publish(device, record=True):
    """End of a frame: copy the guard words (range maxima + the trunk's error word) into pinned host memory, asynchronously on
    the current stream.  ``record=False`` inside a stream capture (an event recorded there is a graph node, not something the host
    can query): the caller marks the replay's end with ``guards_mark``."""
    st = _range_state(device)      # (with RANGE_GUARD off the range words stay zero; the two error words of the spin kernels are still mirrored)
    st["mirror"].copy_(st["buf"], non_blocking=True)
    if record:
        guards_mark(device)


def guards_mark(device):
    st = _range_state(device)
    st["event"].record(torch.cuda.current_stream())
    st["pending"] = True


def guards_poll(device):
    """Start of a frame: look at what the PREVIOUS frame published -- a plain read of pinned memory, no synchronisation (if that
    copy has not landed yet it is looked at a frame later).  Marks new hot producers (returned) and raises if a dataflow-trunk
    launch timed out."""
    st = _range_state(device)
    if not st["pending"] or not st["event"].query():
        return set()
    return _guards_look(st)


def _guards_look(st):
    st["pending"] = False
    words = st["mirror"]
    err = int(words[_TRUNK_ERROR_SLOT])
    if err:
        _trunk_failed(st, err)
    if int(words[_FILL_ERROR_SLOT]):
        _fill_failed(st)
    if not RANGE_GUARD:
        return set()
    return _mark_hot(st, words.view(torch.float32), conservative=True)


def guards_flush(device):
    """END of a sequence (``SuperResolutionPipeline.reset()`` / ``close()``, the end of an offline render): the frame-late look of
    ``guards_poll`` done NOW for the last frame -- waits for that frame's guard-word copy (one event synchronisation, the frame's
    work is what it waits for) and raises / marks exactly like ``guards_poll``.  Without it the last frame of a sequence is never
    followed by a poll."""
    device = _range_device(device)
    st = _range.get(device)
    if st is None or not st["pending"]:
        return set()
    st["event"].synchronize()
    return _guards_look(st)


def range_reset():
    """Forget every maximum, every hot producer and every producer's word (a new model was loaded)."""
    for st in _range.values():
        st["buf"][:_FILL_ERROR_SLOT].zero_()
        st["hot"].clear()
        st["slots"].clear()
        st["members"].clear()
        st["frames"] = 0
        st["pending"] = False
    _routing_changed()           # guard words are handed out anew: a captured launch would keep writing the old ones


def range_check_due(device):
    """Frame pipelines call this once per frame: True for the FIRST frame since the last reset (the synchronous check that makes a
    checkpoint's first frame right); every later frame is covered by ``guards_publish`` / ``guards_poll``."""
    if not RANGE_GUARD:
        return False
    st = _range_state(device)
    st["frames"] += 1
    return st["frames"] == 1


# ---- split-operand mode: fp32-equivalent accuracy on the fp16 matrix pipe (inference; THE default parity path) ----------
# SPLIT_F16 = True routes the no-grad ``conv3x3`` of layers with more than 8 output channels through
# ``isrConv3x3ForwardSplit`` (csrc/sr_conv_split.hip): every operand is split into two fp16 numbers (22 significand
# bits), a product is three fp16 MFMAs accumulated in fp32 -- 5.3x fewer matrix cycles than the fp32 MFMA at an error
# against fp64 that matches the exact fp32 kernel's (tests/test_conv_gpu.py).  SPLIT_F16 = False restores the exact
# k-ordered fmaf-chain kernels of sr_conv3x3.hip (training always uses those).
SPLIT_F16 = True
_split_cache = _WeightImages()


def _prepare_split(weight, transpose_flip=False):
    """Weights as scaled (hi, lo) fp16 pairs in the split kernel's layout, cached like ``prepare_weights``;
    transpose_flip: the data-gradient weights w'[ci][co][ky][kx] = w[co][ci][2-ky][2-kx]."""
    lib = _sr()

    def build():
        w = weight.detach().contiguous()
        cout, cin = w.shape[0], w.shape[1]
        if not transpose_flip:
            wq = torch.empty(lib.isrConvSplitWeightBytes(cin, cout), dtype=torch.uint8, device=weight.device)
            return wq, lib.isrConvSplitPrepare(_ptr(w), _ptr(wq), cout, cin, _stream())
        wq = torch.empty(lib.isrConvSplitWeightBytes(cout, cin), dtype=torch.uint8, device=weight.device)
        return wq, lib.isrConvSplitPrepareMany(1, (ctypes.c_void_p * 1)(w.data_ptr()), None, (ctypes.c_void_p * 1)(wq.data_ptr()),
                                               (ctypes.c_int * 1)(cout), (ctypes.c_int * 1)(cin), _stream())
    return _split_cache.get((id(weight), bool(transpose_flip)), (weight,), build, "isrConvSplitPrepareMany" if transpose_flip else "isrConvSplitPrepare")


def _split_cached(weight, transpose_flip):
    return _split_cache.lookup((id(weight), bool(transpose_flip)), (weight,)) is not None


def prepare_split_many(weights):
    """Bring the cached split-kernel images (forward AND data gradient) of all given [Cout, Cin, 3, 3] weights up to date in
    two launches (``isrConvSplitPrepareMany``).  A training step changes every weight, and preparing them one by one costs two
    launches per image -- ~100 small launches per step for EnhanceNet."""
    lib = _sr()
    stale = [w for w in weights if w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3)
             and w.is_contiguous() and not (_split_cached(w, False) and _split_cached(w, True))]
    most = lib.isrConvSplitPrepareManyMax()
    for k in range(0, len(stale), most):
        part = stale[k:k + most]
        n = len(part)
        fwd = [torch.empty(lib.isrConvSplitWeightBytes(w.shape[1], w.shape[0]), dtype=torch.uint8, device=w.device) for w in part]
        bwd = [torch.empty(lib.isrConvSplitWeightBytes(w.shape[0], w.shape[1]), dtype=torch.uint8, device=w.device) for w in part]
        pw = (ctypes.c_void_p * n)(*[w.data_ptr() for w in part])
        pf = (ctypes.c_void_p * n)(*[t.data_ptr() for t in fwd])
        pb = (ctypes.c_void_p * n)(*[t.data_ptr() for t in bwd])
        co = (ctypes.c_int * n)(*[w.shape[0] for w in part])
        ci = (ctypes.c_int * n)(*[w.shape[1] for w in part])
        rc = lib.isrConvSplitPrepareMany(n, pw, pf, pb, co, ci, _stream())
        if rc != 0:
            raise RuntimeError("isrConvSplitPrepareMany failed (%d)" % rc)
        for w, f, b in zip(part, fwd, bwd):
            _split_cache.store((id(w), False), (w,), f)
            _split_cache.store((id(w), True), (w,), b)


def _split_fits(x, cout, upsample2x):
    """The split kernels address one image through 32-bit buffer offsets: input and output of a launch must each stay
    below 2 GiB (the caller falls back to the exact fp32 kernels otherwise)."""
    h, w = (2 * x.shape[2], 2 * x.shape[3]) if upsample2x else (x.shape[2], x.shape[3])
    xplane = max(x.stride(1), x.shape[2] * x.shape[3]) if x.stride(3) == 1 else x.shape[2] * x.shape[3]
    return x.shape[1] * xplane * 4 < 2 ** 31 and cout * (h * w + plane_pad(h, w)) * 4 < 2 ** 31


def conv3x3_split(x, weight, bias=None, act='none', slope=0.01, residual=None, upsample2x=False):
    """``conv3x3`` on the split-operand kernel (no autograd): y = act(conv3x3(U(x), w) + bias) + residual."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    with torch.no_grad():
        key = _arm_range(id(weight), x.device)
        y = _launch_lp("isrConv3x3ForwardSplit", x, _prepare_split(weight), bias.contiguous() if bias is not None else None, residual,
                       weight.shape[0], act, slope, upsample2x)
        y._isr_range_key = key
        return y


# ---- mixed-precision training mode (opt-in, NOT the parity path) ------------------------------------------------------
# TRAIN_BF16 = True runs the forward and data-gradient convolutions of the autograd functions below with bf16 MFMA
# operands (fp32 accumulation, fp32 tensors, fp32 master weights; the weight gradients and everything else stay
# fp32).  bf16 rather than fp16: gradients span the fp32 exponent range.  Layers with at most 8 input or output
# channels (the 64 -> 6 output layer and its data gradient) keep their fp32 kernels.
TRAIN_BF16 = False
# Forward and data-gradient convolutions of the training graph on the split-operand kernels (csrc/sr_conv_split.hip:
# three fp16 MFMAs per product on (hi, lo) operand pairs, fp32 accumulation -- the fp32 kernels' accuracy against fp64,
# NOT a reduced-precision mode) for layers with at least TRAIN_SPLIT_MIN_TILES tiles of 8x32 pixels; smaller layers and
# all weight gradients stay on the exact fp32 MFMA kernels.
TRAIN_SPLIT = True
# GATE_FUSION: a conv3x3 whose input is the output of a ReLU conv3x3 applies that ReLU's backward in the epilogue of its own
# data gradient (one isrActBackward launch and a 3-tensor round trip less per such pair).  Parameter and input gradients are
# bit-identical either way; the gradient of the INTERMEDIATE activation is then the post-gate value -- a tensor hook or
# retain_grad() on it switches the fusion off for that pair (tests/test_train_kernels_gpu.py), torch.autograd.grad on it does not.
GATE_FUSION = True
TRAIN_SPLIT_MIN_TILES = 256
TRAIN_SPLIT_FEW_INPUTS = os.environ.get("ISR_TRAIN_SPLIT_FEW_INPUTS", "1") != "0"
TRAIN_SPLIT_MIN_TILES2 = 128      # small images: 2-row tiles (the library picks that form below 256 tiles of 8x32 pixels)


def _train_conv(x, weight, transpose_flip, bias, residual, act):
    """Forward (or, with transpose_flip, data-gradient) convolution of the training graph.  Results are PACKED
    tensors: they are saved for backward and their raw pointers go to ``isrActBackward`` and the weight-gradient
    kernels, which index [N, C, H, W] flat (inference outputs may have padded channel planes, these never do)."""
    cout, cin = (weight.shape[1], weight.shape[0]) if transpose_flip else (weight.shape[0], weight.shape[1])
    # the low-precision kernel is a streaming kernel with 8x32-pixel x 64-channel tiles: it pays from a few hundred
    # tiles on (the 128x128 layers of a crop batch); below that the fp32 kernels' finer decompositions are faster
    tiles = x.shape[0] * ((x.shape[2] + 7) // 8) * ((x.shape[3] + 31) // 32)
    flops = 2.0 * 9 * cin * cout * x.shape[0] * x.shape[2] * x.shape[3]
    if TRAIN_BF16 and cout > 8 and cin > 8 and tiles >= 256:
        _tally("bf16", flops)
        return _launch_lp("isrConv3x3ForwardBf16", x, _prepare_lp(weight, transpose_flip, True), bias, residual, cout, act, 0.0, False, packed=True)
    # the split-operand kernel (fp32-equivalent accuracy, 2.3x the fp32 MFMA kernel) once a layer has enough 8x32-pixel
    # tiles to fill the persistent grid: the 64^2 / 128^2 post-block layers of a crop batch, 54 % of the step's flops
    # ... or, for a batch of small crops, enough 2-row tiles for the small-image form (conv3x3_split_rows2_kernel)
    tiles2 = x.shape[0] * ((x.shape[2] + 1) // 2) * ((x.shape[3] + 31) // 32)
    # (few INPUT channels are fine -- the 6 -> 64 data gradient of the output layer is one k-step of mostly zero padding, a store-bound
    # launch -- few OUTPUT channels are not: the 32-row MFMA tile would be mostly padding, conv3x3_small_cout_kernel takes those)
    if TRAIN_SPLIT and cout > 8 and (cin > 8 or TRAIN_SPLIT_FEW_INPUTS) and (tiles >= TRAIN_SPLIT_MIN_TILES or tiles2 >= TRAIN_SPLIT_MIN_TILES2) \
            and x.shape[3] % 4 == 0 and _split_fits(x, cout, False):
        _tally("split", flops)
        slot = _gmax_slot(x.device, _GMAX_CONV_WORDS) if transpose_flip else None    # a data gradient: some layer's gz later on
        if slot is not None:
            _sr().isrSetMaxSlots(ctypes.c_void_p(slot), _GMAX_CONV_WORDS)
        y = _launch_lp("isrConv3x3ForwardSplit", x, _prepare_split(weight, transpose_flip), bias, residual, cout, act, 0.0, False, packed=True)
        if slot is not None:
            words = _sr().isrTakeMaxSlotWords()
            if words > 0:
                _gmax_tag(y, slot, words)
        return y
    _tally("exact", flops)
    return _launch_forward(x, prepare_weights(weight, transpose_flip=transpose_flip), bias, residual, cin, cout, act, 0.0, False,
                           packed=True)


# Optional tally of the algorithmic flops a step dispatches to each kernel family ("split": three fp16 MFMAs per product,
# ceiling 2500 / 3 TFLOP/s; "exact": fp32 MFMA, ceiling 157.3): bench.py --mode train prices its roofline with it.
FLOP_TALLY = None


def _tally(family, flops):
    if FLOP_TALLY is not None:
        FLOP_TALLY[family] = FLOP_TALLY.get(family, 0.0) + float(flops)


_workspace = {}


def _wgrad_workspace(device, nbytes):
    ws = _workspace.get(device)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _workspace[device] = ws
    return ws


def _wgrad_kind(xs, gzs, weight):
    """Which weight-gradient kernels take these pairs.  "bf16" (the mixed-precision mode) and "split" need enough 4x32-pixel tiles to
    stream (the kernels are memory bound), W % 4 == 0 and 16-byte aligned gradients; everything else is "exact"."""
    n, _, h, w = xs[0].shape
    tiles = n * len(xs) * ((h + 3) // 4) * ((w + 31) // 32)
    big = w % 4 == 0 and tiles >= 1024 and all(t.data_ptr() % 16 == 0 for t in gzs)
    if TRAIN_BF16 and big and weight.shape[0] > 8:
        return "bf16"
    # (the split kernel also takes the 64 -> 6 output layer: its 32-row MFMA tile is mostly padding there, but at a
    # fifth of the matrix cycles it still beats the fp32 K-split kernel)
    return "split" if (TRAIN_SPLIT and big) else "exact"


def _wgrad_segments(xs, gzs, weight, dw, db, accumulate=0):
    """One weight-gradient pass over at most 32 pairs (xs[k], gzs[k]) into dw / db; returns the entry point's code.  The split kind
    takes the maxima the producers of gzs left behind (``_gmax_of``) and ``accumulate`` (bit 0: dw +=, bit 1: db +=)."""
    lib = _sr()
    cout, cin = weight.shape[0], weight.shape[1]
    n, _, h, w = xs[0].shape
    kind = _wgrad_kind(xs, gzs, weight)
    if accumulate and kind != "split":
        raise RuntimeError("only the split-operand weight gradient accumulates")
    ws = _wgrad_workspace(weight.device, lib.isrConvWeightGradWorkspace(n, cin, h, w, cout))
    px = (ctypes.c_void_p * len(xs))(*[t.data_ptr() for t in xs])
    pg = (ctypes.c_void_p * len(gzs))(*[t.data_ptr() for t in gzs])
    _tally(kind, 2.0 * 9 * cin * cout * n * len(xs) * h * w)
    shape = (_ptr(ws), n, cin, h, w, cout, _stream())
    if kind != "split":
        fn = lib.isrConv3x3WeightGradSegmentsBf16 if kind == "bf16" else lib.isrConv3x3WeightGradSegments
        return fn(px, pg, len(xs), _ptr(dw), _ptr(db), *shape)
    maxima = [_gmax_of(t) for t in gzs]
    tagged = all(m is not None for m in maxima) and len(set(m[1] for m in maxima)) == 1
    pm = (ctypes.c_void_p * len(gzs))(*[m[0] for m in maxima]) if tagged else None
    return lib.isrConv3x3WeightGradSegmentsSplitMax(px, pg, pm, maxima[0][1] if tagged else 0, len(xs), _ptr(dw), _ptr(db), accumulate, *shape)


def _weight_grad(xs, gzs, weight, has_bias):
    """(dw, db) summed over the pairs (xs[k], gzs[k]) -- ``isrConv3x3WeightGradSegments``, one pass per <= 32 pairs."""
    most = _sr().isrConvWeightGradMaxSegments()
    gw = gb = None
    for k in range(0, len(xs), most):
        dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
        db = torch.empty(weight.shape[0], dtype=torch.float32, device=weight.device) if has_bias else None
        rc = _wgrad_segments(xs[k:k + most], gzs[k:k + most], weight, dw, db)
        if rc != 0:
            raise RuntimeError("isrConv3x3WeightGradSegments failed (%d)" % rc)
        gw = dw if gw is None else gw + dw
        gb = db if gb is None or db is None else gb + db
    return gw, gb


# Deferred weight gradients.  The frames of a training clip run the SAME layers one after the other, and backward
# through time visits them again in reverse: per layer that is T weight-gradient launches over few pixels each (a
# 32x32 crop batch fills a quarter of the GPU), T slab reductions and T-1 accumulations into .grad.  Inside
# ``deferred_weight_gradients()`` the backward of ``conv3x3`` only records (input, output gradient) and returns no
# weight gradient; leaving the context runs ONE weight-gradient pass per layer over all recorded frames and adds the
# result to ``weight.grad`` / ``bias.grad`` -- the same sums in another order.
_deferred = None
# The split-operand weight gradient scales gz by a power of two taken from max |gz| over the launch's tensors: a pass over every
# gradient tensor.  Inside deferred_weight_gradients() the kernels that PRODUCE those tensors -- the fused small-image block
# (isrResBlockSmall, backward direction: both outputs) and the persistent split-operand convolution (isrSetMaxSlots) -- leave the
# maxima of their outputs in words of a per-step pool instead (one word per wave, no contention), the tensors are tagged with the words' address, and a layer whose gz tensors all carry a valid tag skips the pass
# (isrConv3x3WeightGradSegmentsSplitMax).  The same maxima, the same scale: bit-identical gradients.
GMAX_FROM_PRODUCERS = os.environ.get("ISR_GMAX_FROM_PRODUCERS", "1") != "0"
_GMAX_WORDS = 1 << 20
_GMAX_CONV_WORDS = 8192    # isrSetMaxSlots capacity: 4 words per workgroup (up to four per CU on the one-workgroup-per-tile form)
_gmax = None              # {"pool": int32 tensor, "next": int} of the active deferred_weight_gradients() context


def _gmax_slot(device, words):
    """Address of `words` zeroed words for the maxima of a gradient tensor, or None (outside the context / switched off / pool used up)."""
    global _gmax
    if _deferred is None or not GMAX_FROM_PRODUCERS:
        return None
    if _gmax is None:
        _gmax = {"pool": torch.zeros(_GMAX_WORDS, dtype=torch.int32, device=device), "next": 0}
    if _gmax["pool"].device != device or _gmax["next"] + words > _GMAX_WORDS:
        return None
    _gmax["next"] += words
    return _gmax["pool"].data_ptr() + 4 * (_gmax["next"] - words)


def _gmax_tag(t, slot, words):
    t._isr_gmax = (slot, words, t.data_ptr(), t._version, _gmax["pool"])      # the pool lives as long as a tag points into it


def _gmax_of(t):
    tag = getattr(t, '_isr_gmax', None)
    if tag is None or tag[2] != t.data_ptr() or tag[3] != t._version or _gmax is None or tag[4] is not _gmax["pool"]:
        return None
    return tag[0], tag[1]


class deferred_weight_gradients:
    def __enter__(self):
        global _deferred, _gmax
        if _deferred is not None:
            raise RuntimeError("deferred_weight_gradients() does not nest")
        _deferred = {}
        _gmax = None
        return self

    def __exit__(self, exc_type, exc, tb):
        global _deferred, _gmax
        pending, _deferred = _deferred, None
        try:
            return self._finish(pending, exc_type)
        finally:
            _gmax = None

    @staticmethod
    def _finish(pending, exc_type):
        if exc_type is not None:
            return False
        for key, (weight, bias, xs, gzs) in pending.items():
            if len(key) > 2 and key[2] == "s2":      # a stride-2 convolution: its own weight-gradient kernel
                gw, gb = _conv_s2_weight_grad(xs, gzs, weight, bias is not None)
            elif len(key) > 2:       # a transposed convolution: (x, phase-major gradient) pairs, the gradient gathered into its own layout
                gw, gb = _convt_weight_grad(xs, gzs, weight, bias is not None)
            elif _weight_grad_into_grad(xs, gzs, weight, bias):
                continue
            else:
                gw, gb = _weight_grad(xs, gzs, weight, bias is not None)
            for param, g in ((weight, gw), (bias, gb)):
                if param is None or g is None or not param.requires_grad:
                    continue
                if param.grad is None:
                    param.grad = g.view_as(param)
                else:
                    param.grad.add_(g.view_as(param))
        return False


# The deferred pass writes straight into .grad: a layer that takes the split-operand kernel in one piece (<= 32 frames) has its slab
# reduction ADD to the parameters' gradients (the `accumulate` argument of isrConv3x3WeightGradSegmentsSplitMax) instead of producing dw / db for a `grad += dw` launch per
# parameter (47 launches per step).  Same sums, same roundings (tests/test_train_kernels_gpu.py).  (Tried: the weight-gradient kernels
# of all layers back to back and ONE reduction launch at the end -- 71 launches fewer, the same step time: the slabs, 38 MB per layer,
# then come back from memory instead of the caches.)
WGRAD_INTO_GRAD = os.environ.get("ISR_WGRAD_INTO_GRAD", "1") != "0"


def _weight_grad_into_grad(xs, gzs, weight, bias):
    """The layer's weight (and bias) gradient added to ``weight.grad`` / ``bias.grad`` by the reduction itself; False: not eligible."""
    if not (WGRAD_INTO_GRAD and not TRAIN_BF16 and len(xs) <= _sr().isrConvWeightGradMaxSegments()
            and _wgrad_kind(xs, gzs, weight) == "split"):
        return False
    bits = 0
    for k, param in enumerate((weight, bias)):
        if param is None:
            continue
        if not param.requires_grad or (param.grad is not None and not param.grad.is_contiguous()):
            return False
        if param.grad is None:
            param.grad = torch.empty_like(param, memory_format=torch.contiguous_format)
        else:
            bits |= 1 << k
    rc = _wgrad_segments(xs, gzs, weight, weight.grad, bias.grad if bias is not None else None, bits)
    if rc != 0:
        raise RuntimeError("isrConv3x3WeightGradSegmentsSplitMax failed (%d)" % rc)
    return True


def _has_grad_hooks(p):
    return p is not None and bool(getattr(p, '_backward_hooks', None) or getattr(p, '_post_accumulate_grad_hooks', None))


def _weight_grad_or_defer(weight, bias, has_bias, x, gz, convt=False, s2=False):
    """Inside deferred_weight_gradients(): record the pair and return (None, None); else compute (dw, db) now.
    ``convt``: ``weight`` is a ConvTranspose2d weight [ci, co, 3, 3] and ``gz`` the phase-major gradient (``_convt_weight_grad``).
    ``s2``: the layer is a stride-2 convolution, ``gz`` has half of x's size (``_conv_s2_weight_grad``).

    Deferred gradients are written to ``param.grad`` when the context exits, AFTER ``loss.backward()`` and without
    passing through autograd's accumulation: tensor hooks and post-accumulate-grad hooks (DDP-style reducers,
    per-parameter clipping / logging) would never fire and ``torch.autograd.grad(..., weights)`` would see None.  A
    parameter that carries such hooks is therefore NOT deferred (its gradient is computed here, per frame, and flows
    through autograd as usual); ``torch.autograd.grad`` on convolution weights must be called outside the context."""
    if _deferred is not None and weight.is_leaf and (bias is None or bias.is_leaf) \
            and not _has_grad_hooks(weight) and not _has_grad_hooks(bias):
        key = (id(weight), tuple(x.shape), "convt") if convt else (id(weight), tuple(x.shape), "s2") if s2 else (id(weight), tuple(x.shape))
        entry = _deferred.setdefault(key, (weight, bias, [], []))
        entry[2].append(x)
        entry[3].append(gz)
        return None, None
    return (_convt_weight_grad if convt else _conv_s2_weight_grad if s2 else _weight_grad)([x], [gz], weight, has_bias)


# A residual block of a batch of SMALL images (the 32 x 32 training crops: too few 8 x 32 tiles for the streaming kernel) as ONE
# launch forward and ONE backward (csrc/sr_conv_block2.h: both convolutions, the intermediate's halo rows recomputed per 2-row
# tile) instead of two each: bit-identical tensors, one chain of launch latencies instead of two.
TRAIN_BLOCK2 = os.environ.get("ISR_TRAIN_BLOCK2", "1") != "0"


def _block2_supported(x, w1, w2):
    n, c, h, w = x.shape
    if not (TRAIN_BLOCK2 and TRAIN_SPLIT and not TRAIN_BF16 and c == 64 and tuple(w1.shape) == (64, 64, 3, 3) and tuple(w2.shape) == (64, 64, 3, 3)):
        return False
    if n * ((h + 7) // 8) * ((w + 31) // 32) >= TRAIN_SPLIT_MIN_TILES or n * ((h + 1) // 2) < TRAIN_SPLIT_MIN_TILES2:
        return False                        # enough 8 x 32 tiles for the streaming kernel / too few rows to fill the GPU
    return bool(_sr().isrResBlockSmallSupported(n, h, w))


def _block2(x, wa, ba, gate, wb, bb, transpose_flip):
    """(z, y): z = relu(conv(x, wa) + ba) (or, with ``gate``: conv(x, wa) where gate > 0, else 0), y = conv(z, wb) + bb + x;
    x, gate: packed [N, 64, H, W]."""
    n, _, h, w = x.shape
    z, y = torch.empty_like(x), torch.empty_like(x)
    _tally("split", 2 * 2.0 * 9 * 64 * 64 * n * h * w)
    words = 4 * n * ((h + 1) // 2)                                     # one per wave of the launch
    zs = _gmax_slot(x.device, words) if transpose_flip else None      # data gradients: both outputs are some layer's gz
    ys = _gmax_slot(x.device, words) if (transpose_flip and zs is not None) else None
    if ys is None:
        zs = None
    rc = _sr().isrResBlockSmall(_ptr(x), _ptr(_prepare_split(wa, transpose_flip)), _ptr(ba), _ptr(gate), _ptr(_prepare_split(wb, transpose_flip)),
                                _ptr(bb), _ptr(z), _ptr(y), n, h, w, ctypes.c_void_p(zs), ctypes.c_void_p(ys), _stream())
    if rc != 0:
        raise RuntimeError("isrResBlockSmall failed (%d)" % rc)
    if zs is not None:
        _gmax_tag(z, zs, words)
        _gmax_tag(y, ys, words)
    return z, y


class _ResidualBlockFunction(torch.autograd.Function):
    """y = x + conv2(relu(conv1(x))) -- EnhanceNet's residual block (enhancenet.py:18-33,141) as ONE autograd node of
    two fused launches forward and two backward: the data gradient of conv2 is gated by relu's output in its epilogue
    (ISR_ACT_GATE) and the data gradient of conv1 adds the skip path's gradient in its epilogue, where separate
    nodes need an activation-backward launch and an accumulation launch in between."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x = x.contiguous()
        if _block2_supported(x, w1, w2):
            t, y = _block2(x, w1, b1.contiguous() if b1 is not None else None, None, w2, b2.contiguous() if b2 is not None else None, False)
        else:
            t = _train_conv(x, w1, False, b1.contiguous() if b1 is not None else None, None, 'relu')
            y = _train_conv(t, w2, False, b2.contiguous() if b2 is not None else None, x, 'none')
        ctx.params = (w1, b1, w2, b2)
        ctx.save_for_backward(x, t)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, t = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        gy = gy.contiguous()
        gx = None
        if ctx.needs_input_grad[0] and _block2_supported(gy, w1, w2):
            gz1, gx = _block2(gy, w2, None, t, w1, None, True)
        else:
            gz1 = _train_conv(gy, w2, True, None, t, 'gate')
            if ctx.needs_input_grad[0]:
                gx = _train_conv(gz1, w1, True, None, gy, 'none')
        gw1 = gb1 = gw2 = gb2 = None
        if ctx.needs_input_grad[3] or (b2 is not None and ctx.needs_input_grad[4]):
            gw2, gb2 = _weight_grad_or_defer(w2, b2 if (b2 is not None and b2.requires_grad) else None, b2 is not None, t, gy)
        if ctx.needs_input_grad[1] or (b1 is not None and ctx.needs_input_grad[2]):
            gw1, gb1 = _weight_grad_or_defer(w1, b1 if (b1 is not None and b1.requires_grad) else None, b1 is not None, x, gz1)
        return gx, gw1, gb1, gw2, gb2


# ---- the whole low-resolution trunk as ONE dataflow launch (csrc/sr_conv_trunk.hip) -----------------------------------------
# preblock + the residual blocks of a single image whose tiles all fit on the GPU at once (<= #CUs tiles of 16 x 32 pixels, one
# workgroup per CU: the 480 x 270 frame has 255): workgroup w owns tile w through every layer and waits only for its 3 x 3
# neighbourhood's progress.  Bit-identical to the per-layer launches.  Every tile must be RESIDENT: a co-runner that holds a CU (a
# second process on the device, another stream's kernel) can keep a tile out, its neighbours' waits then run into the 50 ms
# deadline, the launch ends with an incomplete output and the error word set.  That word is one of the per-frame guard words:
# ``guards_poll`` at the start of the next frame raises and switches the dataflow form off for the process (``trunk_check()`` is the
# synchronous look: bench.py after its timed region, tests).  Do not use it on a shared device (bench.py: BENCH_SHARE_DEVICE).
TRUNK_DATAFLOW = os.environ.get("ISR_TRUNK_DATAFLOW", "1") != "0"
_trunk_ws = {}


def trunk_supported(x, convs):
    """x [1, Cin, h, w]; convs: [(weight, bias)] = preblock, then conv1 / conv2 of every block."""
    if not (TRUNK_DATAFLOW and not DEVICE_SHARED and SPLIT_F16 and not FAST_F16 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1):
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(w.requires_grad for w, _ in convs)):
        return False
    if len(convs) < 1 or len(convs) % 2 != 1 or len(convs) > 24 or tuple(convs[0][0].shape[2:]) != (3, 3) or convs[0][0].shape[0] != 64:
        return False
    if any(tuple(w.shape) != (64, 64, 3, 3) for w, _ in convs[1:]) or convs[0][0].shape[1] != x.shape[1]:
        return False
    if any_hot(x.device) or range_is_hot(getattr(x, '_isr_range_key', None), x.device):
        return False
    xs, xp, _ = _plane_strides(x)
    return xs is x and bool(_sr().isrTrunkDataflowSupported(_ptr(x), x.shape[1], x.shape[2], x.shape[3], xp, x.shape[2] * x.shape[3] + plane_pad(x.shape[2], x.shape[3])))


def _trunk_workspace(device, cin, h, w):
    """The dataflow trunk's workspace for this size on the current stream: header (zero unit, the tiles' progress counters, error
    word) + the packed-split input, F and T tensors of the launch; zero-filled once."""
    key = (device, cin, h, w, torch.cuda.current_stream().cuda_stream)
    ws = _trunk_ws.get(key)
    if ws is None:
        ws = torch.zeros(_sr().isrTrunkDataflowWorkspaceBytes(cin, h, w) // 4, dtype=torch.int32, device=device)
        _trunk_ws[key] = ws
    return ws


def trunk_dataflow(x, convs):
    """f = relu(conv(x, w0) + b0); f = f + conv(relu(conv(f, w1) + b1), w2) + b2; ...  in ONE launch (``isrTrunkDataflow``)."""
    lib = _sr()
    prepacked = getattr(x, '_isr_prepacked', None)
    x, xp, _ = _plane_strides(x)
    _, cin, h, w = x.shape
    ws = _trunk_workspace(x.device, cin, h, w)
    if prepacked is not None and prepacked is not ws:
        raise RuntimeError("trunk_dataflow: the input was assembled into another workspace (another stream?) than this launch uses")
    f = empty_planes(1, 64, h, w, x.device)
    wq = [_prepare_split(wt) for wt, _ in convs]
    bs = [b.detach().contiguous() if b is not None else None for _, b in convs]
    n = len(convs)
    pw = (ctypes.c_void_p * n)(*[q.data_ptr() for q in wq])
    pb = (ctypes.c_void_p * n)(*[(b.data_ptr() if b is not None else None) for b in bs])
    st = _range_state(x.device)
    lib.isrSetTrunkErrorWord(ctypes.c_void_p(st["buf"].data_ptr() + 4 * _TRUNK_ERROR_SLOT))
    f._isr_range_key = _arm_range(("trunk", id(convs[0][0])), x.device, members=[id(wt) for wt, _ in convs])
    lib.isrSetTrunkPackedResult(1 if UPS_PHASE else 0)
    if prepacked is not None:
        # assemble_input_packed left the input packed-split in the workspace: no packing pass
        rc = lib.isrTrunkDataflowPrepacked(cin, _ptr(f), f.stride(1), pw, pb, (n - 1) // 2, h, w, _ptr(ws), _stream())
    else:
        rc = lib.isrTrunkDataflow(_ptr(x), cin, xp, _ptr(f), f.stride(1), pw, pb, (n - 1) // 2, h, w, _ptr(ws), _stream())
    if rc != 0:
        raise RuntimeError("isrTrunkDataflow failed (%d)" % rc)
    # the same result PACKED-SPLIT, inside the workspace (valid until the next launch on it): what the phase-decomposed upsampling
    # layer stages by LDS-DMA (conv3x3_ups_phase)
    off, plane = ctypes.c_longlong(), ctypes.c_longlong()
    if UPS_PHASE and lib.isrTrunkDataflowPackedResult(cin, h, w, ctypes.byref(off), ctypes.byref(plane)) == 0:
        ps = PackedSplit(ws[off.value // 4: off.value // 4 + 2 * 8 * plane.value * 4], 64, h, w, plane.value)
        ps.range_key = f._isr_range_key
        f._isr_packed = ps
    return f


def _trunk_failed(st, err):
    global TRUNK_DATAFLOW
    st["buf"][_TRUNK_ERROR_SLOT] = 0           # sticky on the device: an error of ANY launch since the last look was still there
    TRUNK_DATAFLOW = False                      # whoever catches this goes on with the per-layer kernels
    _routing_changed()                          # ... and a captured frame that holds the dataflow launch is stale (pipeline._graph_signature)
    raise RuntimeError("trunk_dataflow_kernel: a tile timed out waiting for its neighbours at layer %d in a launch since the last "
                       "look (that launch's output is incomplete; a workgroup was not resident -- is the device shared?).  The "
                       "dataflow trunk is now off for this process (ops.TRUNK_DATAFLOW)" % (err - 1))


def trunk_check():
    """Host read of the dataflow launches' error word (ONE synchronisation): raises if a tile ever gave up waiting for a
    neighbour -- which would mean a workgroup was not resident (more tiles than the GPU holds) or the launch was disturbed."""
    for st in list(_range.values()):
        err = int(st["buf"][_TRUNK_ERROR_SLOT].item())
        if err:
            _trunk_failed(st, err)


# Inference: the whole block in ONE launch (csrc/sr_conv_block.hip) -- bit-identical to the two split-operand launches
BLOCK_FUSION = os.environ.get("ISR_BLOCK_FUSION", "0") == "1"
BLOCK_PACKED = os.environ.get("ISR_BLOCK_PACKED", "1") != "0"       # two launches per block, the intermediate packed-split (see residual_block)
BLOCK_PACKED_MIN_TILES = 256
BLOCK_FUSION_MIN_TILES = 256       # below that the persistent grid is not filled; the per-layer kernels' small-image forms take over
_block_ws = {}


def _block_supported(x, w1, w2):
    if not (BLOCK_FUSION and SPLIT_F16 and not FAST_F16 and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[0] == 1):
        return False
    if any_hot(x.device):
        return False
    if tuple(w1.shape) != (64, 64, 3, 3) or tuple(w2.shape) != (64, 64, 3, 3) or x.shape[1] != 64:
        return False
    if ((x.shape[2] + 7) // 8) * ((x.shape[3] + 31) // 32) < BLOCK_FUSION_MIN_TILES:
        return False
    xs, xp, _ = _plane_strides(x)
    return xs is x and bool(_sr().isrResBlockSplitSupported(_ptr(x), x.shape[2], x.shape[3], xp, x.shape[2] * x.shape[3] + plane_pad(x.shape[2], x.shape[3])))


def residual_block_fused(x, w1, b1, w2, b2):
    """x + conv3x3(relu(conv3x3(x, w1, b1)), w2, b2) for one [1, 64, H, W] image in one launch of ``isrResBlockSplit``."""
    lib = _sr()
    x, xp, _ = _plane_strides(x)
    _, _, h, w = x.shape
    key = (x.device, torch.cuda.current_stream().cuda_stream)
    ws = _block_ws.get(key)
    if ws is None:
        ws = torch.empty(lib.isrResBlockSplitWorkspaceBytes(), dtype=torch.uint8, device=x.device)
        _block_ws[key] = ws
    y = empty_planes(1, 64, h, w, x.device)
    y._isr_range_key = _arm_range(("block", id(w1)), x.device, members=[id(w1), id(w2)])      # covers the intermediate and the output
    rc = lib.isrResBlockSplit(_ptr(x), _ptr(_prepare_split(w1)), _ptr(b1.detach().contiguous() if b1 is not None else None),
                              _ptr(_prepare_split(w2)), _ptr(b2.detach().contiguous() if b2 is not None else None), _ptr(y), _ptr(ws),
                              h, w, xp, y.stride(1), _stream())
    if rc != 0:
        raise RuntimeError("isrResBlockSplit failed (%d)" % rc)
    return y


def residual_block(x, w1, b1, w2, b2):
    """x + conv3x3(relu(conv3x3(x, w1, b1)), w2, b2), 64 -> 64 -> 64 channels."""
    needs_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w1, b1, w2, b2))
    if x.is_cuda and needs_grad and x.dtype == torch.float32 and w1.shape[0] == w1.shape[1] == w2.shape[0] == w2.shape[1]:
        return _ResidualBlockFunction.apply(x, w1, b1, w2, b2)
    if not needs_grad and _block_supported(x, w1, w2):
        return residual_block_fused(x, w1, b1, w2, b2)
    if not needs_grad and BLOCK_PACKED and SPLIT_F16 and not FAST_F16 and x.is_cuda and x.dtype == torch.float32 and x.shape[0] == 1 \
            and tuple(w1.shape) == (64, 64, 3, 3) == tuple(w2.shape) and x.shape[3] % 4 == 0 \
            and ((x.shape[2] + 7) // 8) * ((x.shape[3] + 31) // 32) >= BLOCK_PACKED_MIN_TILES and packed_supported(x, w1, False):
        # the intermediate of the block travels packed-split: conv1 stores (hi, lo') units straight from its accumulators (no LDS
        # transposition), conv2 stages them by LDS-DMA (no conversion) -- the same numbers, bit-identical output
        t = conv3x3_split_packed(x, w1, b1, act='relu')
        return conv3x3_split_from_packed(t, w2, b2, residual=x)
    return conv3x3(conv3x3(x, w1, b1, act='relu'), w2, b2, residual=x)


class _Conv3x3Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, act, slope):
        # x is the output of a ReLU convolution (tagged by conv3x3 below): the data gradient of THIS layer can then apply
        # that ReLU's backward in its epilogue (ISR_ACT_GATE on x > 0) and the producer skips its isrActBackward launch
        ctx.x_relu = bool(getattr(x, '_isr_relu_out', False)) and x.is_contiguous()
        x = x.contiguous()
        res = residual.contiguous() if residual is not None else None
        b = bias.contiguous() if bias is not None else None
        cout, cin = weight.shape[0], weight.shape[1]
        if cout <= 8 and cin * x.shape[2] * x.shape[3] * 4 < 2 ** 31:
            _tally("exact", 2.0 * 9 * cin * cout * x.shape[0] * x.shape[2] * x.shape[3])
            y = _launch_small(x, weight, b, res, act, slope)      # the 64 -> 6 output layer: 4x4x1 MFMA blocks
        elif act == 'leaky':
            _tally("exact", 2.0 * 9 * cin * cout * x.shape[0] * x.shape[2] * x.shape[3])
            y = _launch_forward(x, prepare_weights(weight), b, res, cin, cout, act, slope, False, packed=True)
        else:
            y = _train_conv(x, weight, False, b, res, act)
        ctx.act, ctx.slope = act, slope
        ctx.has_bias, ctx.has_res = bias is not None, residual is not None
        ctx.bias = bias if (bias is not None and bias.requires_grad) else None
        ctx.weight = weight
        if act != 'none' and residual is not None:
            raise RuntimeError("conv3x3: activation together with a fused residual is inference-only")
        ctx.save_for_backward(x, weight, y if act != 'none' else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _sr()
        x, weight, y = ctx.saved_tensors
        gy = gy.contiguous()
        cout, cin = weight.shape[0], weight.shape[1]
        if ctx.act == 'relu' and getattr(gy, '_isr_gated_by', None) == (y.data_ptr(), y._version, gy._version):
            gz = gy              # the consumer's data gradient already multiplied by (y > 0), see below
        elif ctx.act != 'none':
            gz = torch.empty_like(gy)
            rc = lib.isrActBackward(_ptr(gy), _ptr(y), _ptr(gz), gy.numel(), ACT_CODES[ctx.act], float(ctx.slope), _stream())
            if rc != 0:
                raise RuntimeError("isrActBackward failed (%d)" % rc)
        else:
            gz = gy
        gx = gw = gb = gres = None
        if ctx.needs_input_grad[0]:
            # data gradient = the same fused kernel on flipped / transposed weights
            # (a hook or retain_grad() on x wants dL/dx itself, not dL/dx already multiplied by (x > 0): no fusion then.  What
            # cannot be seen from here -- torch.autograd.grad(loss, x) on the intermediate activation -- gets the gated value)
            if ctx.x_relu and GATE_FUSION and not _has_grad_hooks(x) and not x.retains_grad:
                gx = _train_conv(gz, weight, True, None, x, 'gate')
                gx._isr_gated_by = (x.data_ptr(), x._version, gx._version)   # read by the backward of the layer that produced x
            else:
                gx = _train_conv(gz, weight, True, None, None, 'none')
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _weight_grad_or_defer(ctx.weight, ctx.bias, ctx.has_bias, x, gz)
        if ctx.has_res and ctx.needs_input_grad[3]:
            gres = gy
        return gx, gw, gb, gres, None, None


def _act_cpu(z, act, slope):
    if act == 'relu':
        return F.relu(z)
    if act == 'leaky':
        return F.leaky_relu(z, slope)
    return z


def conv3x3(x, weight, bias=None, act='none', slope=0.01, residual=None, upsample2x=False):
    """See module docstring.  x [N,Cin,h,w], weight [Cout,Cin,3,3] -> [N,Cout,H,W]."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    if not x.is_cuda:
        if upsample2x:
            x = F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
        y = _act_cpu(F.conv2d(x, weight, bias, padding=1), act, slope)
        return y + residual if residual is not None else y
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("conv3x3 (HIP) computes in fp32")
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or
                                              (bias is not None and bias.requires_grad) or
                                              (residual is not None and residual.requires_grad))
    if not needs_grad:
        cout, cin = weight.shape[0], weight.shape[1]
        if FAST_F16 and cout > 8:
            return conv3x3_f16(x, weight, bias, act, slope, residual, upsample2x)
        hot_in = range_is_hot(getattr(x, '_isr_range_key', None), x.device) or \
            (residual is not None and getattr(residual, '_isr_range_key', None) == HOT)
        if SPLIT_F16 and cout > 8 and _split_fits(x, cout, upsample2x) and not hot_in:
            return conv3x3_split(x, weight, bias, act, slope, residual, upsample2x)
        if hot_in and cout > 8:
            # the input (or something upstream of it) came close to the fp16 range of the split: exact fp32 kernel, and whatever
            # consumes ITS output stays exact too (its range is not tracked)
            y = _launch_forward(x, prepare_weights(weight), bias.contiguous() if bias is not None else None, residual,
                                cin, cout, act, slope, upsample2x)
            y._isr_range_key = HOT
            return y
        if cout <= 8 and not upsample2x and cin * x.shape[2] * x.shape[3] * 4 < 2 ** 31:
            return _launch_small(x, weight, bias, residual.contiguous() if residual is not None else None, act, slope)
        if cout <= 8 and not upsample2x:
            _warn_once("small_cout_2g", "conv3x3: %d x %d x %d input exceeds the small-Cout kernel's 2 GiB addressing; the layer "
                       "runs on the general fp32 MFMA kernel (output channels padded to 32)" % (cin, x.shape[2], x.shape[3]))
        return _launch_forward(x, prepare_weights(weight),
                               bias.contiguous() if bias is not None else None,
                               residual,
                               cin, cout, act, slope, upsample2x)
    if upsample2x:   # training: the resize stays its own differentiable op (isrUpsample2xForward / Backward)
        x = bilinear_upsample2x(x)
    if residual is not None and act != 'none':
        return _Conv3x3Function.apply(x, weight, bias, None, act, slope) + residual
    y = _Conv3x3Function.apply(x, weight, bias, residual, act, slope)
    if act == 'relu' and residual is None:
        y._isr_relu_out = True      # a consumer conv3x3 may fold this ReLU's backward into its data gradient
    return y


# ---- stride-2 transposed convolution: TecoGAN's learned x2 upsampling (csrc/sr_conv_transpose.hip) --------------------------------
_convt_cache = _WeightImages(64)


def _prepare_convt(weight, layout="split"):
    """The [ci, co, 3, 3] weight of a ConvTranspose2d(64, 64, 3, 2, 1, 1) as the split kernel's image, cached like ``_prepare_split``.
    ``layout``: "split" the forward kernel's image, "dgrad" the data-gradient kernel's (ci and co trade places)."""
    lib = _sr()
    name = "isrConvTransposeDataGrad" if layout == "dgrad" else "isrConvTransposeSplit"

    def build():
        wq = torch.empty(getattr(lib, name + "WeightBytes")(), dtype=torch.uint8, device=weight.device)
        return wq, getattr(lib, name + "Prepare")(_ptr(weight.detach().contiguous()), _ptr(wq), _stream())
    return _convt_cache.get((id(weight), layout), (weight,), build, name + "Prepare")


_CONVT_TAPS = {0: ((1, 1),), 1: ((1, 2), (2, 0))}                 # phase bit -> ((r, k), ...): embedded row / column r holds tap k


def conv_transpose_phase_weight(weight):
    """The transposed convolution as an ordinary 3x3 convolution with 4 Cout outputs followed by ``F.pixel_shuffle(., 2)``:
    [4 co + 2 a + b][ci][r][s] holds the taps of output phase (a, b) -- w[ci][co][ky][kx] at r = 1 for ky = 1 (a = 0) and ky = 2
    (a = 1), at r = 2 for ky = 0 (a = 1); columns alike -- and zeros elsewhere.  The convolution's zero padding below and to the right
    is the transposed convolution's missing neighbour.  No arithmetic: the same products, four of nine taps structural zeros."""
    cin, cout = weight.shape[0], weight.shape[1]
    w = weight.detach().permute(1, 0, 2, 3)                       # [co, ci, ky, kx]
    e = torch.zeros((cout, 4, cin, 3, 3), dtype=weight.dtype, device=weight.device)
    taps = {0: ((1, 1),), 1: ((1, 2), (2, 0))}                     # phase bit -> ((r, k), ...)
    for a in (0, 1):
        for b in (0, 1):
            for r, ky in taps[a]:
                for s, kx in taps[b]:
                    e[:, 2 * a + b, :, r, s] = w[:, :, ky, kx]
    return e.reshape(4 * cout, cin, 3, 3)


def conv_transpose_weight_from_phase(dwe):
    """The exact adjoint of ``conv_transpose_phase_weight``: [4 co, ci, 3, 3] (the gradient of the embedded weight) -> [ci, co, 3, 3],
    the 9 live taps of 36 gathered -- every (ky, kx) sits at exactly one (phase, r, s); the 27 structural zeros' gradients are dropped.
    No arithmetic."""
    cout, cin = dwe.shape[0] // 4, dwe.shape[1]
    d = dwe.reshape(cout, 4, cin, 3, 3)
    live = {}
    for a in (0, 1):
        for b in (0, 1):
            for r, ky in _CONVT_TAPS[a]:
                for s, kx in _CONVT_TAPS[b]:
                    live[3 * ky + kx] = d[:, 2 * a + b, :, r, s]
    return torch.stack([live[t] for t in range(9)], dim=0).permute(2, 1, 0).reshape(cin, cout, 3, 3).contiguous()


def _convt_embedded(weight, bias):
    """(We [4 co, ci, 3, 3], be [4 co] or None): ``conv_transpose_phase_weight`` and the bias repeated per phase, cached."""
    key = (id(weight), "embed")
    hit = _convt_cache.lookup(key, (weight, bias))
    if hit is None:
        hit = (conv_transpose_phase_weight(weight), bias.detach().repeat_interleave(4).contiguous() if bias is not None else None)
        _convt_cache.store(key, (weight, bias), hit)
    return hit


def _conv_transpose_exact(x, weight, bias, act, slope):
    """The exact fp32 route: the zero-embedded weight on the exact ``isrConv3x3Forward`` kernel, then the pixel shuffle."""
    we, be = _convt_embedded(weight, bias)
    y = _launch_forward(x, prepare_weights(we), be, None, we.shape[1], we.shape[0], act, slope, False, packed=True)
    return F.pixel_shuffle(y, 2)


def _convt_weight_grad(xs, gs, weight, has_bias):
    """(dW [ci, co, 3, 3], db [co]) of a transposed convolution summed over the pairs (xs[k] [N, ci, h, w], gs[k] the phase-major
    gradient [N, 4 co, h, w]): the segment kernels of ``_weight_grad`` on the pair as a ci -> 4 co 3x3 layer (4x the needed matrix
    work: 27 of the 36 taps are structural zeros of the embedded weight), then the live taps gathered
    (``conv_transpose_weight_from_phase``) and the bias gradient summed over the four phases."""
    cin, cout = weight.shape[0], weight.shape[1]
    like = weight.detach().new_empty((4 * cout, cin, 3, 3))           # shape and device of the embedded layer (never read)
    dwe, dbe = _weight_grad(xs, gs, like, has_bias)
    return conv_transpose_weight_from_phase(dwe), (dbe.view(cout, 4).sum(dim=1) if dbe is not None else None)


def _convt_fits(x, weight):
    n, cin, h, w = x.shape
    xplane = max(x.stride(1), h * w) if (x.stride(3) == 1 and x.stride(2) == w) else h * w
    return bool(_sr().isrConvTranspose3x3S2SplitSupported(cin, weight.shape[1], h, w, xplane, 4 * h * w + plane_pad(2 * h, 2 * w)))


def conv_transpose3x3_s2_split(x, weight, bias=None, act='none', slope=0.01):
    """``conv_transpose3x3_s2`` on the split-operand kernel (no autograd; 64 -> 64 channels): one launch per image."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    lib = _sr()
    with torch.no_grad():
        n, cin, h, w = x.shape
        cout = weight.shape[1]
        x, xp, xi = _plane_strides(x)
        wq = _prepare_convt(weight)
        b = bias.detach().contiguous() if bias is not None else None
        y = empty_planes(n, cout, 2 * h, 2 * w, x.device)
        key = None
        for k in range(n):
            key = _arm_range(id(weight), x.device)
            rc = lib.isrConvTranspose3x3S2ForwardSplit(ctypes.c_void_p(x.data_ptr() + 4 * k * xi), _ptr(wq), _ptr(b),
                                                       ctypes.c_void_p(y.data_ptr() + 4 * k * y.stride(0)), cin, h, w, cout,
                                                       ACT_CODES[act], float(slope), xp, y.stride(1), _stream())
            if rc != 0:
                raise RuntimeError("isrConvTranspose3x3S2ForwardSplit failed (%d)" % rc)
        y._isr_range_key = key
        return y


# Training route of the transposed convolution: "kernel" -- the dedicated forward and data-gradient kernels (csrc/sr_conv_transpose.hip);
# "embedded" -- forward and data gradient as the zero-embedded 64 -> 256 3x3 layer on the convolution's own training kernels
# (``_train_conv``: 4x the matrix work); "torch" -- PyTorch's own transposed convolution under autograd, with its warning (the route
# before these kernels existed).  The last two are what tools/bench_tecogan_train.py measures the kernels against.  The weight gradient
# takes the embedded form on both HIP routes.  With TRAIN_SPLIT off both are the embedded layer on the exact fp32 kernels.
CONVT_TRAIN_ROUTE = os.environ.get("ISR_CONVT_TRAIN_ROUTE", "kernel")


def _convt_train_kernel(n, h, w):
    return bool(TRAIN_SPLIT and CONVT_TRAIN_ROUTE == "kernel" and _sr().isrConvTranspose3x3S2SplitSupported(64, 64, h, w, h * w, 4 * h * w)
                and _sr().isrConvTranspose3x3S2DataGradSplitSupported(n, 64, h, w))


def conv_transpose_phase_gradient(gy, y=None, act='none', slope=0.01):
    """The PHASE-MAJOR gradient of a stride-2 transposed convolution's output: G[n, 4 c + 2 a + b, i, j] = gz[n, c, 2i + a, 2j + b] with
    gz = gy act'(y) by the rule of ``isrActBackward`` (gy where y > 0, gy * slope elsewhere; slope 0 for 'relu') -- that launch followed
    by ``F.pixel_unshuffle(., 2)``, as ONE element-wise kernel (``isrConvTransposePhaseGradient``) on device tensors; CPU tensors: the
    definition.  gy, y: [N, C, 2h, 2w]; y may be None with act 'none'."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    if act != 'none' and y is None:
        raise ValueError("conv_transpose_phase_gradient: the activation's backward needs y")
    n, c, hh, ww = gy.shape
    if hh % 2 or ww % 2:
        raise ValueError("conv_transpose_phase_gradient: even height and width expected")
    if not gy.is_cuda:
        gz = gy if act == 'none' else torch.where(y > 0, gy, gy * (0.0 if act == 'relu' else slope))
        return torch.stack([gz[:, :, a::2, b::2] for a in (0, 1) for b in (0, 1)], dim=2).reshape(n, 4 * c, hh // 2, ww // 2)
    if gy.dtype != torch.float32:
        raise TypeError("conv_transpose_phase_gradient (HIP) computes in fp32")
    gy = gy.contiguous()
    y = y.contiguous() if act != 'none' else None
    g = torch.empty((n, 4 * c, hh // 2, ww // 2), dtype=torch.float32, device=gy.device)
    rc = _sr().isrConvTransposePhaseGradient(_ptr(gy), _ptr(y), _ptr(g), n, c, hh // 2, ww // 2, ACT_CODES[act], float(slope), _stream())
    if rc != 0:
        raise RuntimeError("isrConvTransposePhaseGradient failed (%d)" % rc)
    return g


def _convt_data_grad(g, weight):
    """gx [N, 64, h, w] from the phase-major gradient g [N, 256, h, w] (packed) on ``convt3x3s2_dgrad_split_kernel``.  Inside
    ``deferred_weight_gradients()`` the launch leaves the maxima of gx in the per-step words, as the split data gradient of
    ``_train_conv`` does: gx is some layer's gz later on."""
    lib = _sr()
    n, _, h, w = g.shape
    _tally("split", 2.0 * 9 * 64 * 64 * n * h * w)
    gx = torch.empty((n, 64, h, w), dtype=torch.float32, device=g.device)
    slot = _gmax_slot(g.device, _GMAX_CONV_WORDS)
    if slot is not None:
        lib.isrSetMaxSlots(ctypes.c_void_p(slot), _GMAX_CONV_WORDS)
    rc = lib.isrConvTranspose3x3S2DataGradSplit(_ptr(g), _ptr(_prepare_convt(weight, "dgrad")), _ptr(gx), n, 64, h, w, _stream())
    if rc != 0:
        raise RuntimeError("isrConvTranspose3x3S2DataGradSplit failed (%d)" % rc)
    if slot is not None:
        words = lib.isrTakeMaxSlotWords()
        if words > 0:
            _gmax_tag(gx, slot, words)
    return gx


def _convt_data_grad_embedded(g, weight, bias):
    """The same gradient as the data gradient of the zero-embedded 64 -> 256 layer on the convolution's own training kernels."""
    return _train_conv(g, _convt_embedded(weight, bias)[0], True, None, None, 'none')


class _ConvTranspose3x3S2Function(torch.autograd.Function):
    """y = act(conv_transpose2d(x, w, b, 2, 1, 1)) for 64 -> 64 channels as ONE autograd node on the HIP training kernels: forward
    ``isrConvTranspose3x3S2ForwardSplitBatch`` (the inference kernel, the whole batch in one launch; packed output, no range word armed:
    the training rule of ``_train_conv``); backward
    ``isrConvTransposePhaseGradient`` (the activation's backward, written phase-major), ``isrConvTranspose3x3S2DataGradSplit`` and the
    weight gradient of (x, G) as a 64 -> 256 layer through ``_weight_grad_or_defer``."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        lib = _sr()
        x = x.contiguous()
        n, _, h, w = x.shape
        b = bias.detach().contiguous() if bias is not None else None
        if _convt_train_kernel(n, h, w):
            _tally("split", 2.0 * 9 * 64 * 64 * n * h * w)
            wq = _prepare_convt(weight)
            y = torch.empty((n, 64, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
            rc = lib.isrConvTranspose3x3S2ForwardSplitBatch(_ptr(x), _ptr(wq), _ptr(b), _ptr(y), n, h, w, ACT_CODES[act], float(slope), _stream())
            if rc != 0:
                raise RuntimeError("isrConvTranspose3x3S2ForwardSplitBatch failed (%d)" % rc)
        elif TRAIN_SPLIT and CONVT_TRAIN_ROUTE == "embedded" and w % 4 == 0 and _split_fits(x, 256, False):
            _tally("split", 2.0 * 9 * 64 * 256 * n * h * w)
            we, be = _convt_embedded(weight, bias)
            y = F.pixel_shuffle(_launch_lp("isrConv3x3ForwardSplit", x, _prepare_split(we), be, None, 256, act, slope, False, packed=True), 2)
        else:
            _tally("exact", 2.0 * 9 * 64 * 256 * n * h * w)
            y = _conv_transpose_exact(x, weight, bias, act, slope)
        ctx.act, ctx.slope = act, slope
        ctx.has_bias = bias is not None
        ctx.bias_any = bias
        ctx.bias = bias if (bias is not None and bias.requires_grad) else None
        ctx.weight = weight
        ctx.save_for_backward(x, y if act != 'none' else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        weight = ctx.weight
        n, _, h, w = x.shape
        g = conv_transpose_phase_gradient(gy, y, ctx.act, ctx.slope)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            if _convt_train_kernel(n, h, w):
                gx = _convt_data_grad(g, weight)
            else:
                gx = _convt_data_grad_embedded(g, weight, ctx.bias_any)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _weight_grad_or_defer(weight, ctx.bias, ctx.has_bias, x, g, convt=True)
        return gx, gw, gb, None, None


def conv_transpose3x3_s2(x, weight, bias=None, act='none', slope=0.01):
    """y = act(conv_transpose2d(x, w, bias, stride=2, padding=1, output_padding=1)): x [N, Cin, h, w], weight [Cin, Cout, 3, 3] (the
    ``nn.ConvTranspose2d`` layout) -> [N, Cout, 2h, 2w].  TecoGAN's two upsampling layers (64 -> 64).

    * CPU tensors: ``F.conv_transpose2d`` and the activation.
    * device tensors, no gradient needed: the split-operand kernel ``isrConvTranspose3x3S2ForwardSplit`` (csrc/sr_conv_transpose.hip),
      its output armed with a range key like ``conv3x3_split``'s.  With the input's range key hot, ``SPLIT_F16`` off or a shape the
      kernel does not take (channels other than 64, more than 2 GiB): the exact fp32 route -- the four phases as zero-padded 3x3
      taps of a [4 Cout, Cin, 3, 3] weight on the exact ``conv3x3`` kernel, then ``F.pixel_shuffle``.
    * under autograd, device fp32 64 -> 64: ``_ConvTranspose3x3S2Function`` -- forward on the split kernel (packed output; the exact
      embedded route with ``TRAIN_SPLIT`` off or a shape the kernel does not take), backward as the phase-major gradient
      (``isrConvTransposePhaseGradient``), the dedicated split-operand data gradient (``isrConvTranspose3x3S2DataGradSplit``, only when
      the input needs a gradient) and the weight gradient of (x, G) as a 64 -> 256 layer on the convolution's segment kernels, deferred
      inside ``deferred_weight_gradients()`` like every other layer's.  Under ``TRAIN_BF16`` these layers STAY on the split kernels
      (there are no bf16 forms of them).
    * under autograd, other channel counts: PyTorch's own transposed convolution (a warning says so, once)."""
    if act not in ('none', 'relu', 'leaky'):
        raise ValueError("unknown activation %r" % (act,))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or x.shape[1] != weight.shape[0]:
        raise ValueError("conv_transpose3x3_s2: x [N, Cin, h, w] and weight [Cin, Cout, 3, 3] expected")
    if not x.is_cuda:
        return _act_cpu(F.conv_transpose2d(x, weight, bias, stride=2, padding=1, output_padding=1), act, slope)
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("conv_transpose3x3_s2 (HIP) computes in fp32")
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
    if needs_grad and tuple(weight.shape[:2]) == (64, 64) and CONVT_TRAIN_ROUTE != "torch":
        return _ConvTranspose3x3S2Function.apply(x, weight, bias, act, slope)
    if needs_grad:
        _warn_once("convt_autograd", "conv_transpose3x3_s2: under autograd this transposed convolution runs on PyTorch's own kernels "
                   "(the HIP training kernels take 64 -> 64 channels)")
        return _act_cpu(F.conv_transpose2d(x, weight, bias, stride=2, padding=1, output_padding=1), act, slope)
    hot_in = range_is_hot(getattr(x, '_isr_range_key', None), x.device)
    if SPLIT_F16 and not hot_in and _convt_fits(x, weight):
        return conv_transpose3x3_s2_split(x, weight, bias, act, slope)
    with torch.no_grad():
        y = _conv_transpose_exact(x, weight, bias, act, slope)
    if hot_in:
        y._isr_range_key = HOT          # whatever consumes it stays exact too (its range is not tracked)
    return y


# ---- stride-2 convolution: the halving layers of the discriminators (csrc/sr_conv_stride2.hip) -------------------------------------
# Route of ``conv3x3_s2`` on device tensors: "kernel" -- the dedicated forward, data-gradient and weight-gradient kernels; "embedded" --
# the layer as a stride-1 3x3 layer over ``F.pixel_unshuffle(x, 2)`` with 9 of its 36 taps live, on ``conv3x3`` (4x the matrix work: the
# form a layer takes before it has a kernel); "torch" -- PyTorch's own convolution.  The last two are what tools/bench_gan_train.py
# measures the kernels against.
CONV_S2_ROUTE = os.environ.get("ISR_CONV_S2_ROUTE", "kernel")
_CONV_S2_TAPS = ((1, 0), (0, 1), (1, 1))                        # tap k -> (phase bit, embedded row / column): input row 2i + k - 1 = 2 (i + r - 1) + a


def conv_s2_phase_weight(weight):
    """The stride-2 convolution as a stride-1 3x3 convolution over ``F.pixel_unshuffle(x, 2)`` (channel 4 ci + 2 a + b = x[ci] at rows
    2u + a, columns 2v + b): [co][4 ci + 2 a + b][r][s] holds w[co][ci][ky][kx] at (a, r) = (1, 0), (0, 1), (1, 1) for ky = 0, 1, 2, columns
    alike, and zeros elsewhere.  Differentiable in ``weight``; no arithmetic: the same products, 27 of 36 taps structural zeros."""
    cout, cin = weight.shape[0], weight.shape[1]
    e = weight.new_zeros((cout, cin, 4, 3, 3))
    for ky, (a, r) in enumerate(_CONV_S2_TAPS):
        for kx, (b, q) in enumerate(_CONV_S2_TAPS):
            e[:, :, 2 * a + b, r, q] = weight[:, :, ky, kx]
    return e.reshape(cout, 4 * cin, 3, 3)


def conv_s2_supported(x, weight):
    """Do the stride-2 kernels take this layer?  Even sizes, channel counts that are multiples of 16 from 16 to 256."""
    lib = _sr()
    n, cin, h, w = x.shape
    return hasattr(lib, "isrConv3x3S2Forward") and bool(lib.isrConv3x3S2Supported(n, cin, weight.shape[0], h, w))


def _conv_s2_forward(x, weight, bias, act, slope):
    n, cin, h, w = x.shape
    cout = weight.shape[0]
    _tally("exact", 2.0 * 9 * cin * cout * n * (h // 2) * (w // 2))
    y = torch.empty((n, cout, h // 2, w // 2), dtype=torch.float32, device=x.device)
    wd = weight.detach().contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    rc = _sr().isrConv3x3S2Forward(_ptr(x), _ptr(wd), _ptr(b), _ptr(y), n, cin, h, w, cout, ACT_CODES[act], float(slope), _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3S2Forward failed (%d)" % rc)
    return y


def _conv_s2_data_grad(gz, weight, h, w):
    """gx [N, Cin, h, w] from the pre-activation gradient gz [N, Cout, h/2, w/2] (``isrConv3x3S2DataGrad``)."""
    n, cout = gz.shape[0], gz.shape[1]
    cin = weight.shape[1]
    _tally("exact", 2.0 * 9 * cin * cout * n * (h // 2) * (w // 2))
    gx = torch.empty((n, cin, h, w), dtype=torch.float32, device=gz.device)
    rc = _sr().isrConv3x3S2DataGrad(_ptr(gz), _ptr(weight.detach().contiguous()), _ptr(gx), n, cin, h, w, cout, _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3S2DataGrad failed (%d)" % rc)
    return gx


def _conv_s2_weight_grad(xs, gzs, weight, has_bias):
    """(dw, db) of a stride-2 convolution summed over the pairs (xs[k] [N, Cin, h, w], gzs[k] [N, Cout, h/2, w/2]) --
    ``isrConv3x3S2WeightGradSegments``, one pass per <= 32 pairs."""
    lib = _sr()
    most = lib.isrConvWeightGradMaxSegments()
    cout, cin = weight.shape[0], weight.shape[1]
    n, _, h, w = xs[0].shape
    ws = _wgrad_workspace(weight.device, lib.isrConv3x3S2WeightGradWorkspace(n * min(len(xs), most), cin, h, w, cout))
    gw = gb = None
    for k in range(0, len(xs), most):
        px = [t.contiguous() for t in xs[k:k + most]]
        pg = [t.contiguous() for t in gzs[k:k + most]]
        dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
        db = torch.empty(cout, dtype=torch.float32, device=weight.device) if has_bias else None
        _tally("exact", 2.0 * 9 * cin * cout * n * len(px) * (h // 2) * (w // 2))
        rc = lib.isrConv3x3S2WeightGradSegments((ctypes.c_void_p * len(px))(*[t.data_ptr() for t in px]),
                                                (ctypes.c_void_p * len(pg))(*[t.data_ptr() for t in pg]), len(px), _ptr(dw), _ptr(db),
                                                _ptr(ws), n, cin, h, w, cout, _stream())
        if rc != 0:
            raise RuntimeError("isrConv3x3S2WeightGradSegments failed (%d)" % rc)
        gw = dw if gw is None else gw + dw
        gb = db if gb is None or db is None else gb + db
    return gw, gb


class _Conv3x3S2Function(torch.autograd.Function):
    """y = act(conv2d(x, w, b, stride=2, padding=1)) as ONE autograd node on the stride-2 kernels: forward ``isrConv3x3S2Forward``;
    backward ``isrActBackward`` on the saved output, ``isrConv3x3S2DataGrad`` (only when the input needs a gradient) and the weight
    gradient through ``_weight_grad_or_defer`` (``isrConv3x3S2WeightGradSegments``, deferred over the frames of a clip)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, slope):
        x = x.contiguous()
        y = _conv_s2_forward(x, weight, bias, act, slope)
        ctx.act, ctx.slope = act, slope
        ctx.has_bias = bias is not None
        ctx.bias = bias if (bias is not None and bias.requires_grad) else None
        ctx.weight = weight
        ctx.save_for_backward(x, y if act != 'none' else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y = ctx.saved_tensors
        weight = ctx.weight
        gy = gy.contiguous()
        if ctx.act != 'none':
            gz = torch.empty_like(gy)
            rc = _sr().isrActBackward(_ptr(gy), _ptr(y), _ptr(gz), gy.numel(), ACT_CODES[ctx.act], float(ctx.slope), _stream())
            if rc != 0:
                raise RuntimeError("isrActBackward failed (%d)" % rc)
        else:
            gz = gy
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _conv_s2_data_grad(gz, weight, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            gw, gb = _weight_grad_or_defer(weight, ctx.bias, ctx.has_bias, x, gz, s2=True)
        return gx, gw, gb, None, None


def conv3x3_s2(x, weight, bias=None, act='none', slope=0.01):
    """y = act(conv2d(x, w, bias, stride=2, padding=1)): x [N, Cin, H, W], weight [Cout, Cin, 3, 3] -> [N, Cout, H/2, W/2]; ``act`` is
    'none' or 'leaky'.  The halving layers of the discriminators (losses/enhancenetsmall.py, enhancenetlarge.py).

    * CPU tensors: ``F.conv2d`` and the activation.
    * device fp32 tensors, no gradient needed: the forward kernel ``isrConv3x3S2Forward`` (exact fp32 MFMA, nine products per pixel).
    * under autograd: ``_Conv3x3S2Function`` -- that forward, ``isrActBackward``, ``isrConv3x3S2DataGrad`` when the input needs a
      gradient, and the weight gradient (``isrConv3x3S2WeightGradSegments``) deferred inside ``deferred_weight_gradients()`` like
      every other layer's.
    * ``CONV_S2_ROUTE``: "embedded" runs the layer as ``conv3x3`` over the pixel-unshuffled input, "torch" on PyTorch's convolution.
    * odd sizes, channel counts that are no multiple of 16 or exceed 256: PyTorch's convolution (a warning says so, once)."""
    if act not in ('none', 'leaky'):
        raise ValueError("conv3x3_s2: activation 'none' or 'leaky' expected, not %r" % (act,))
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or x.shape[1] != weight.shape[1]:
        raise ValueError("conv3x3_s2: x [N, Cin, H, W] and weight [Cout, Cin, 3, 3] expected")
    if not x.is_cuda:
        return _act_cpu(F.conv2d(x, weight, bias, stride=2, padding=1), act, slope)
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("conv3x3_s2 (HIP) computes in fp32")
    if CONV_S2_ROUTE not in ("kernel", "embedded", "torch"):
        raise ValueError("ops.CONV_S2_ROUTE: 'kernel', 'embedded' or 'torch' expected, not %r" % (CONV_S2_ROUTE,))
    if CONV_S2_ROUTE == "torch":
        return _act_cpu(F.conv2d(x, weight, bias, stride=2, padding=1), act, slope)
    if x.shape[2] % 2 or x.shape[3] % 2 or (CONV_S2_ROUTE == "kernel" and not conv_s2_supported(x, weight)):
        if CONV_S2_ROUTE == "kernel" and not hasattr(_sr(), "isrConv3x3S2Forward"):
            raise RuntimeError("conv3x3_s2: the loaded kernel library has no stride-2 convolution (isrConv3x3S2Forward)")
        _warn_once("conv_s2_shape", "conv3x3_s2: %d -> %d channels at %d x %d runs on PyTorch's own convolution (the HIP kernels take even "
                   "sizes and channel counts that are multiples of 16 up to 256)" % (x.shape[1], weight.shape[0], x.shape[2], x.shape[3]))
        return _act_cpu(F.conv2d(x, weight, bias, stride=2, padding=1), act, slope)
    if CONV_S2_ROUTE == "embedded":
        return conv3x3(F.pixel_unshuffle(x, 2), conv_s2_phase_weight(weight), bias, act=act, slope=slope)
    needs_grad = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or (bias is not None and bias.requires_grad))
    if needs_grad:
        return _Conv3x3S2Function.apply(x, weight, bias, act, slope)
    return _conv_s2_forward(x.contiguous(), weight, bias, act, slope)


# ---- training-side elementwise kernels (csrc/sr_train.hip) ---------------------------------------
class _Upsample2xFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        n, c, h, w = x.shape
        y = torch.empty((n, c, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        rc = _sr().isrUpsample2xForward(_ptr(x), _ptr(y), n * c, h, w, _stream())
        if rc != 0:
            raise RuntimeError("isrUpsample2xForward failed (%d)" % rc)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        n, c, H, W = gy.shape
        gx = torch.empty((n, c, H // 2, W // 2), dtype=torch.float32, device=gy.device)
        rc = _sr().isrUpsample2xBackward(_ptr(gy), _ptr(gx), n * c, H // 2, W // 2, _stream())
        if rc != 0:
            raise RuntimeError("isrUpsample2xBackward failed (%d)" % rc)
        return gx


def bilinear_upsample2x(x):
    """``F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)`` with a hand-written forward and
    (gather, deterministic) backward on the GPU; PyTorch's launch takes ~340 us for a 64-channel 64^2 -> 128^2 batch
    of 16 that moves 84 MB."""
    if not x.is_cuda:
        return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)
    if x.dtype != torch.float32:
        raise TypeError("bilinear_upsample2x (HIP) computes in fp32")
    return _Upsample2xFunction.apply(x)


class _ReconResidualFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, outputs, inputs, k):
        outputs, inputs = outputs.contiguous(), inputs.contiguous()
        n, cout, H, W = outputs.shape
        cin, h, w = inputs.shape[1], inputs.shape[2], inputs.shape[3]
        out = torch.empty_like(outputs)
        rc = _sr().isrReconResidualForward(_ptr(outputs), _ptr(inputs), _ptr(out), n, cout, cin, k, h, w, _stream())
        if rc != 0:
            raise RuntimeError("isrReconResidualForward failed (%d)" % rc)
        ctx.dims = (n, cout, cin, k, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        n, cout, cin, k, h, w = ctx.dims
        g = g.contiguous()
        gin = None
        if ctx.needs_input_grad[1]:
            gin = torch.empty((n, cin, h, w), dtype=torch.float32, device=g.device)
            rc = _sr().isrReconResidualBackward(_ptr(g), _ptr(gin), n, cout, cin, k, h, w, _stream())
            if rc != 0:
                raise RuntimeError("isrReconResidualBackward failed (%d)" % rc)
        return g, gin, None


def recon_residual_supported(outputs, inputs, k):
    return (outputs.is_cuda and outputs.dtype == torch.float32 and inputs.dtype == torch.float32 and outputs.dim() == 4
            and outputs.shape[0] == inputs.shape[0] and outputs.shape[2] == 4 * inputs.shape[2] and outputs.shape[3] == 4 * inputs.shape[3]
            and 0 < k <= min(outputs.shape[1], inputs.shape[1]) and outputs.shape[0] <= 65535 and outputs.shape[2] <= 65535)


def recon_residual(outputs, inputs, k):
    """``outputs`` with the bilinearly x4-resized first ``k`` channels of ``inputs`` added to its first ``k`` channels
    (EnhanceNet's residual reconstruction) in one launch; differentiable w.r.t. both."""
    return _ReconResidualFunction.apply(outputs, inputs, k)


def _batch_view(t, c, h, w):
    """(tensor, batch stride in floats) of a [B, c, h, w] view whose images are packed (a frame of a [B, T, ..] clip)."""
    if t.stride(3) == 1 and t.stride(2) == w and t.stride(1) == h * w and (t.shape[0] == 1 or t.stride(0) >= c * h * w):
        return t, (t.stride(0) if t.shape[0] > 1 else c * h * w)
    t = t.contiguous()
    return t, c * h * w


class _RecurrentInputFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prev_raw, input_low, flow_low):
        prev_raw = prev_raw.contiguous()
        b, _, h, w = input_low.shape
        inp, istride = _batch_view(input_low, 5, h, w)
        flo, fstride = _batch_view(flow_low, 2, h, w)
        netin = torch.empty((b, 101, h, w), dtype=torch.float32, device=prev_raw.device)
        warped = torch.empty((b, 6, 4 * h, 4 * w), dtype=torch.float32, device=prev_raw.device)
        rc = _sr().isrRecurrentInputForward(_ptr(prev_raw), _ptr(inp), _ptr(flo), _ptr(netin), _ptr(warped), b, h, w,
                                            istride, fstride, _stream())
        if rc != 0:
            raise RuntimeError("isrRecurrentInputForward failed (%d)" % rc)
        ctx.save_for_backward(prev_raw, flo)
        ctx.fstride = fstride
        return netin, warped

    @staticmethod
    def backward(ctx, g_netin, g_warped):
        prev_raw, flo = ctx.saved_tensors
        b, _, H, W = prev_raw.shape
        g_netin = g_netin.contiguous() if g_netin is not None else None
        g_warped = g_warped.contiguous() if g_warped is not None else None
        scratch = torch.empty_like(prev_raw)
        g_raw = torch.empty_like(prev_raw)
        rc = _sr().isrRecurrentInputBackward(_ptr(prev_raw), _ptr(flo), _ptr(g_netin), _ptr(g_warped), _ptr(scratch), _ptr(g_raw),
                                             b, H // 4, W // 4, ctx.fstride, _stream())
        if rc != 0:
            raise RuntimeError("isrRecurrentInputBackward failed (%d)" % rc)
        return g_raw, None, None


def recurrent_input(prev_raw, input_low, flow_low):
    """Network input of frame t > 0 of a training clip and the warped previous frame the temp-l2 loss compares against:
    (net_input [B,101,h,w], warped [B,6,4h,4w]) from the RAW prediction of frame t-1 [B,6,4h,4w], the frame's low-res
    input [B,5,h,w] and the flow [B,2,h,w]; differentiable w.r.t. prev_raw.  Replaces clamp / normalize / cat,
    ``VideoTools.warp_upscale(.., special_mask=True)``, ``VideoTools.flatten_high`` and the final cat (~25 launches
    forward, ~35 backward) by one launch forward and three backward."""
    return _RecurrentInputFunction.apply(prev_raw, input_low, flow_low)


def recurrent_input_supported(prev_raw, input_low, flow_low, upscale):
    return (upscale == 4 and prev_raw.is_cuda and prev_raw.dtype == torch.float32 and input_low.dtype == torch.float32
            and prev_raw.shape[1] == 6 and input_low.shape[1] == 5 and not flow_low.requires_grad and not input_low.requires_grad
            and prev_raw.shape[2] == 4 * input_low.shape[2] and prev_raw.shape[3] == 4 * input_low.shape[3])


def _aligned16(t):
    """``t`` (contiguous, or None) at a 16-byte aligned address: itself, or a copy where it is a view at an odd storage offset --
    ``.contiguous()`` keeps such a view as it is, and the loss kernels read quads of pixels with 16-byte loads."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


LOSS_KINDS = ('mse', 'l1', 'temp-l2')
LOSS_TARGETS = ('mask', 'normal', 'ao', 'depth', 'color')
_loss_ws = {}


class _LossUnshadedFunction(torch.autograd.Function):
    """values[16] = the 15 term means + the weighted total, see ``isrLossUnshadedForward``."""

    @staticmethod
    def forward(ctx, gt, pred, prev, cfg):
        lib = _sr()
        gt, pred = _aligned16(gt.contiguous()), _aligned16(pred.contiguous())
        prev = _aligned16(prev.contiguous()) if prev is not None else None
        n, _, h, w = pred.shape
        key = (pred.device, torch.cuda.current_stream().cuda_stream)
        ws = _loss_ws.get(key)
        if ws is None:
            ws = torch.empty(lib.isrLossUnshadedWorkspace(), dtype=torch.uint8, device=pred.device)
            _loss_ws[key] = ws
        values = torch.empty(16, dtype=torch.float32, device=pred.device)
        rc = lib.isrLossUnshadedForward(_ptr(gt), _ptr(pred), _ptr(prev), n, h, w, cfg['pad'], cfg['weights'], cfg['enabled'],
                                        cfg['shading'], cfg['ao'], cfg['inverse_ao'], _ptr(ws), _ptr(values), _stream())
        if rc != 0:
            raise RuntimeError("isrLossUnshadedForward failed (%d)" % rc)
        ctx.cfg = cfg
        ctx.save_for_backward(gt, pred, prev)
        return values

    @staticmethod
    def backward(ctx, gvalues):
        lib = _sr()
        gt, pred, prev = ctx.saved_tensors
        cfg = ctx.cfg
        n, _, h, w = pred.shape
        gvalues = gvalues.contiguous()
        gpred = torch.empty_like(pred)
        gprev = torch.empty_like(prev) if prev is not None and ctx.needs_input_grad[2] else None
        rc = lib.isrLossUnshadedBackward(_ptr(gt), _ptr(pred), _ptr(prev), n, h, w, cfg['pad'], cfg['weights'], cfg['enabled'],
                                         cfg['shading'], cfg['ao'], cfg['inverse_ao'], _ptr(gvalues), _ptr(gpred), _ptr(gprev),
                                         _stream())
        if rc != 0:
            raise RuntimeError("isrLossUnshadedBackward failed (%d)" % rc)
        return None, gpred, gprev, None


def loss_unshaded_config(weight_dict, padding, shading):
    """Host-side constants of the fused loss: weight_dict {(kind, target): weight}, shading = the loss module's
    ScreenSpaceShading (specular must be off)."""
    weights = [0.0] * 15
    enabled = 0
    for (kind, target), wgt in weight_dict.items():
        kind = 'mse' if kind in ('l2', 'l2_loss') else kind
        t = LOSS_KINDS.index(kind) * 5 + LOSS_TARGETS.index(target)
        weights[t] = float(wgt)
        enabled |= 1 << t
    v = shading.packed_parameters()          # ambient, diffuse, specular, light, material, background
    amb, diff, light, mat, bg = v[0:3], v[3:6], v[9:12], v[12:15], v[15:18]
    sh = [a * m for a, m in zip(amb, mat)] + [d * m for d, m in zip(diff, mat)] + list(light) + list(bg)
    return {'pad': int(padding), 'weights': (ctypes.c_float * 15)(*weights), 'enabled': enabled,
            'shading': (ctypes.c_float * 12)(*sh), 'ao': float(shading._ao), 'inverse_ao': int(bool(shading.inverse_ao))}


def loss_unshaded(gt, pred, prev, cfg):
    """-> values[16] (differentiable w.r.t. pred and prev through values[15], the weighted total)."""
    return _LossUnshadedFunction.apply(gt, pred, prev, cfg)


# ---- downsample-consistency terms l2-ds / l1-ds (csrc/sr_train.hip: loss_downsample_kernel) --------------------------------------
LOSS_DS_KINDS = ('l2-ds', 'l1-ds')
LOSS_DS_TARGETS = ('mask', 'normal', 'depth', 'color')
_loss_ds_ws = {}


def _offset_ptr(t, index):
    return ctypes.c_void_p(t.data_ptr() + index * t.element_size())


class _LossUnshadedDsFunction(torch.autograd.Function):
    """values[24] = the 16 of ``_LossUnshadedFunction``, the ds terms added to [15], + the 8 ds means, see ``isrLossDownsampleForward``.
    ONE node: the ds backward adds into the ``gpred`` that ``isrLossUnshadedBackward`` has just written on the same stream."""

    @staticmethod
    def forward(ctx, gt, pred, prev, input, cfg, ds_cfg):
        lib = _sr()
        gt, pred = _aligned16(gt.contiguous()), _aligned16(pred.contiguous())
        prev = _aligned16(prev.contiguous()) if prev is not None else None
        input = _aligned16(input.contiguous())
        n, _, h, w = pred.shape
        key = (pred.device, torch.cuda.current_stream().cuda_stream)
        ws = _loss_ws.get(key)
        if ws is None:
            ws = torch.empty(lib.isrLossUnshadedWorkspace(), dtype=torch.uint8, device=pred.device)
            _loss_ws[key] = ws
        ds_ws = _loss_ds_ws.get(key)
        if ds_ws is None:
            ds_ws = torch.empty(lib.isrLossDownsampleWorkspace(), dtype=torch.uint8, device=pred.device)
            _loss_ds_ws[key] = ds_ws
        values = torch.empty(24, dtype=torch.float32, device=pred.device)
        rc = lib.isrLossUnshadedForward(_ptr(gt), _ptr(pred), _ptr(prev), n, h, w, cfg['pad'], cfg['weights'], cfg['enabled'],
                                        cfg['shading'], cfg['ao'], cfg['inverse_ao'], _ptr(ws), _ptr(values), _stream())
        if rc != 0:
            raise RuntimeError("isrLossUnshadedForward failed (%d)" % rc)
        rc = lib.isrLossDownsampleForward(_ptr(pred), _ptr(input), n, h, w, ds_cfg['pad'], ds_cfg['weights'], ds_cfg['enabled'],
                                          ds_cfg['shading'], ds_cfg['ao'], ds_cfg['inverse_ao'], _ptr(ds_ws), _offset_ptr(values, 16),
                                          _offset_ptr(values, 15), _stream())
        if rc != 0:
            raise RuntimeError("isrLossDownsampleForward failed (%d)" % rc)
        ctx.cfg, ctx.ds_cfg = cfg, ds_cfg
        ctx.save_for_backward(gt, pred, prev, input)
        return values

    @staticmethod
    def backward(ctx, gvalues):
        lib = _sr()
        gt, pred, prev, input = ctx.saved_tensors
        cfg, ds_cfg = ctx.cfg, ctx.ds_cfg
        n, _, h, w = pred.shape
        gvalues = gvalues.contiguous()
        gpred = torch.empty_like(pred)
        gprev = torch.empty_like(prev) if prev is not None and ctx.needs_input_grad[2] else None
        rc = lib.isrLossUnshadedBackward(_ptr(gt), _ptr(pred), _ptr(prev), n, h, w, cfg['pad'], cfg['weights'], cfg['enabled'],
                                         cfg['shading'], cfg['ao'], cfg['inverse_ao'], _ptr(gvalues), _ptr(gpred), _ptr(gprev),
                                         _stream())
        if rc != 0:
            raise RuntimeError("isrLossUnshadedBackward failed (%d)" % rc)
        rc = lib.isrLossDownsampleBackward(_ptr(pred), _ptr(input), n, h, w, ds_cfg['pad'], ds_cfg['weights'], ds_cfg['enabled'],
                                           ds_cfg['shading'], ds_cfg['ao'], ds_cfg['inverse_ao'], _offset_ptr(gvalues, 15), _ptr(gpred),
                                           _stream())
        if rc != 0:
            raise RuntimeError("isrLossDownsampleBackward failed (%d)" % rc)
        return None, gpred, gprev, None, None, None


def loss_downsample_config(weight_dict, padding, shading):
    """Host-side constants of the ds terms: weight_dict {('l2-ds' | 'l1-ds', target): weight} (other keys are not read), the rest as
    ``loss_unshaded_config``."""
    weights = [0.0] * 8
    enabled = 0
    for (kind, target), wgt in weight_dict.items():
        if kind in LOSS_DS_KINDS:
            t = LOSS_DS_KINDS.index(kind) * 4 + LOSS_DS_TARGETS.index(target)
            weights[t] = float(wgt)
            enabled |= 1 << t
    sh, ao, inv = _discr_shading(shading)
    return {'pad': int(padding), 'weights': (ctypes.c_float * 8)(*weights), 'enabled': enabled, 'shading': sh, 'ao': ao, 'inverse_ao': inv}


def loss_downsample_supported(pred, input, padding):
    """Whether ``loss_unshaded_ds`` has its kernels for these operands: fp32 GPU tensors [N, 6, H, W] and [N, 5, H, W] on one device,
    an input that needs no gradient, a library that has the entry points, H and W multiples of 4 and ``2 * padding < min(H, W)``."""
    if not (torch.is_tensor(pred) and torch.is_tensor(input) and pred.is_cuda and input.is_cuda and pred.device == input.device
            and pred.dtype == torch.float32 and input.dtype == torch.float32 and pred.dim() == 4 and input.dim() == 4
            and pred.shape[1] == 6 and input.shape == (pred.shape[0], 5, pred.shape[2], pred.shape[3]) and not input.requires_grad):
        return False
    lib = _sr()
    return hasattr(lib, "isrLossDownsampleForward") and bool(lib.isrLossDownsampleSupported(pred.shape[0], pred.shape[2], pred.shape[3],
                                                                                            int(padding)))


def loss_unshaded_ds(gt, pred, prev, input, cfg, ds_cfg):
    """``loss_unshaded`` with the downsample-consistency terms -> values[24]: [0..14] as ``loss_unshaded``, [15] the weighted total
    INCLUDING the ds terms, [16..23] the ds means (``LOSS_DS_KINDS`` x ``LOSS_DS_TARGETS``).  Differentiable w.r.t. pred and prev
    through values[15]; ``input`` [N, 5, H, W], the upsampled low-resolution input, gets no gradient."""
    return _LossUnshadedDsFunction.apply(gt, pred, prev, input, cfg, ds_cfg)


# ---- discriminator inputs of the adversarial terms (csrc/sr_train.hip: discr_input_kernel) -------------------------------------
# ISR_DISCR_INPUT_FUSED=0: the torch composition everywhere (A/B runs of tools/bench_gan_train.py)
DISCR_INPUT_FUSED = os.environ.get("ISR_DISCR_INPUT_FUSED", "1") != "0"
_DISCR_CHANNELS = {(True, True, True): 26, (False, False, True): 16, (True, False, False): 13}     # (input, prev_input, prev) present


def pad_border(img, border):
    """Overwrites a ``border``-pixel frame of ``img`` with zeros (size unchanged): ``LossNetUnshaded.pad``."""
    if border == 0:
        return img
    b, c, h, w = img.shape
    inner = img[:, :, border:h - border, border:w - border]
    out = F.pad(inner, (border, border, border, border), 'constant', 0)
    assert out.shape[2] == h and out.shape[3] == w
    return out


def discriminator_part(t, *, padding, shading, order, raw_normal=False, color=None):
    """One 8-channel part of a discriminator input with torch operators, ``t`` [B, 6, H, W]: mask, normalised normal, then colour and
    ao (``order`` 0, the generator side) or ao and colour (``order`` 1, ``train_discriminator``), border zeroed.  The colour is
    ``shading`` of the normalised normal, with ``raw_normal`` of ``t`` as it is; ``color``: that shading where the caller has it."""
    from .utils import ScreenSpaceShading
    assert t.shape[1] == 6
    mask, normal, ao = t[:, 0:1], ScreenSpaceShading.normalize(t[:, 1:4], dim=1), t[:, 5:6]
    if color is None:
        color = shading(t if raw_normal else torch.cat([mask, normal, t[:, 4:6]], dim=1))
    return pad_border(torch.cat([mask, normal, color, ao] if order == 0 else [mask, normal, ao, color], dim=1), padding)


def _discriminator_input_torch(cur, prev, input, prev_input, padding, shading, order, cur_raw_normal):
    parts = [pad_border(t, padding) for t in (input, prev_input) if t is not None]
    parts.append(discriminator_part(cur, padding=padding, shading=shading, order=order, raw_normal=cur_raw_normal))
    if prev is not None:
        parts.append(discriminator_part(prev, padding=padding, shading=shading, order=order))
    return torch.cat(parts, dim=1)


def _discr_operand(t, channels, like):
    return t is None or (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.device == like.device
                         and t.shape == (like.shape[0], channels, like.shape[2], like.shape[3])
                         and (not t.is_contiguous() or t.data_ptr() % 16 == 0))


def discriminator_input_supported(cur, prev=None, input=None, prev_input=None, *, padding, shading=None):
    """Whether ``discriminator_input`` takes the kernel route for these operands: fp32 GPU tensors of one size, one of the three part
    combinations, a width that is a multiple of 4, ``2 * padding < min(H, W)``, 16-byte aligned storage, no specular term."""
    if not (torch.is_tensor(cur) and cur.is_cuda and cur.dim() == 4 and cur.shape[1] == 6 and _discr_operand(cur, 6, cur)):
        return False
    if (input is not None, prev_input is not None, prev is not None) not in _DISCR_CHANNELS:
        return False
    if not (_discr_operand(prev, 6, cur) and _discr_operand(input, 5, cur) and _discr_operand(prev_input, 5, cur)):
        return False
    if shading is not None and shading.enable_specular:
        return False
    n, _, h, w = cur.shape
    return bool(_sr().isrDiscrInputSupported(n, h, w, int(padding)))


_discr_shading_cache = {}


def _discr_shading(shading):
    """(shading12, ao strength, inverse_ao) as the kernels take them (the layout of ``loss_unshaded_config``)."""
    v = shading.packed_parameters()
    key = (tuple(v), float(shading._ao), bool(shading.inverse_ao))
    hit = _discr_shading_cache.get(key)
    if hit is None:
        amb, diff, light, mat, bg = v[0:3], v[3:6], v[9:12], v[12:15], v[15:18]
        sh = [a * m for a, m in zip(amb, mat)] + [d * m for d, m in zip(diff, mat)] + list(light) + list(bg)
        if len(_discr_shading_cache) > 64:
            _discr_shading_cache.clear()
        hit = _discr_shading_cache[key] = ((ctypes.c_float * 12)(*sh), key[1], int(key[2]))
    return hit


class _DiscrInputFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cur, prev, input, prev_input, cfg):
        cur, prev, input, prev_input = (t.contiguous() if t is not None else None for t in (cur, prev, input, prev_input))
        n, _, h, w = cur.shape
        pad, order, raw, (sh, ao, inv) = cfg
        channels = _DISCR_CHANNELS[(input is not None, prev_input is not None, prev is not None)]
        out = torch.empty((n, channels, h, w), dtype=torch.float32, device=cur.device)
        rc = _sr().isrDiscrInputForward(_ptr(input), _ptr(prev_input), _ptr(cur), _ptr(prev), _ptr(out), n, h, w, pad, order, raw, sh, ao, inv,
                                        _stream())
        if rc != 0:
            raise RuntimeError("isrDiscrInputForward failed (%d)" % rc)
        ctx.cfg, ctx.channels = cfg, channels
        ctx.save_for_backward(cur, prev)
        return out

    @staticmethod
    def backward(ctx, gout):
        cur, prev = ctx.saved_tensors
        pad, order, raw, (sh, ao, inv) = ctx.cfg
        n, _, h, w = cur.shape
        gout = gout.contiguous()
        gcur = torch.empty_like(cur)
        gprev = torch.empty_like(prev) if prev is not None and ctx.needs_input_grad[1] else None
        rc = _sr().isrDiscrInputBackward(_ptr(cur), _ptr(prev), _ptr(gout), _ptr(gcur), _ptr(gprev), ctx.channels, n, h, w, pad, order, raw,
                                         sh, ao, inv, _stream())
        if rc != 0:
            raise RuntimeError("isrDiscrInputBackward failed (%d)" % rc)
        return gcur, gprev, None, None, None


def discriminator_input(cur, prev=None, input=None, prev_input=None, *, padding, shading, order, cur_raw_normal):
    """The tensor a discriminator of the adversarial terms reads, [B, 26 | 16 | 13, H, W]: the parts that are given in the order
    ``input``, ``prev_input`` ([B, 5, H, W]: the upsampled input, the warped previous input), then ``discriminator_part`` of ``cur`` and
    of ``prev`` ([B, 6, H, W]), a ``padding``-pixel border zeroed; differentiable w.r.t. ``cur`` and ``prev``.  The operands are passed
    unpadded.  On the GPU one launch forward and one backward (``isrDiscrInputForward`` / ``Backward``) instead of normalise, shade,
    pad and concatenate with torch operators; CPU tensors, shapes the predicate refuses, a shader with its specular term on and
    ``DISCR_INPUT_FUSED = False`` take that composition."""
    if order not in (0, 1):
        raise ValueError("order is 0 (mask, normal, colour, ao) or 1 (mask, normal, ao, colour)")
    if cur.shape[1] != 6:
        raise ValueError("cur is [B, 6, H, W] (mask, normal, depth, ao)")
    if (input is not None, prev_input is not None, prev is not None) not in _DISCR_CHANNELS:
        raise ValueError("a discriminator reads input + prev_input + cur + prev (26 channels), cur + prev (16) or input + cur (13)")
    if DISCR_INPUT_FUSED and discriminator_input_supported(cur, prev, input, prev_input, padding=padding, shading=shading):
        cfg = (int(padding), int(order), int(bool(cur_raw_normal)), _discr_shading(shading))
        return _DiscrInputFunction.apply(cur, prev, input, prev_input, cfg)
    return _discriminator_input_torch(cur, prev, input, prev_input, padding, shading, order, bool(cur_raw_normal))


@contextlib.contextmanager
def graph_capture(graph, **kw):
    """``torch.cuda.graph(graph, **kw)`` with the CYCLIC garbage collector out of the way.

    A global-mode stream capture makes most HIP calls illegal on every thread until it ends.  If a cyclic collection runs
    INSIDE the capture and finalises GPU objects that an earlier caller dropped in a reference cycle (a HIP graph, a
    stream or event of a SuperResolutionPipeline, a cached workspace), their destructors call hipFree / hipEventDestroy /
    hipGraphDestroy from C++ ``noexcept`` code while the capture is open: the runtime reports an error, the destructor
    throws, ``std::terminate`` -- "Fatal Python error: Aborted" with the main thread "Garbage-collecting" (one full GPU
    test run of round 3 died exactly there, in ``GraphedTrainStep.__init__``).  torch 2.10's ``graph.__enter__`` does not
    collect by itself any more.  So: drain the device, collect NOW (destructors run at a quiescent point), and keep the
    collector off until the capture has ended.

    What this does NOT cover (the caller's contract): it removes the cyclic collector, the path that produced the abort.  An
    object whose reference count drops to zero INSIDE the capture body (a stream, event, graph or tensor the body itself lets
    go of) is still finalised there and then, and a collection or a free triggered from ANOTHER thread during the capture is
    not held back either.  Capture bodies in this package (``train.GraphedTrainStep``, ``SuperResolutionPipeline._frame_graph``)
    therefore allocate their streams / events / workspaces before the capture (the eager warm-up pass) and hold them in
    attributes for the graph's lifetime; multi-threaded hosts must not free GPU objects while a capture is open."""
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield graph
    finally:
        if was_enabled:
            gc.enable()


def adam_flat_step(params, grads, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps):
    """One Adam step over flat fp32 buffers (``isrAdamFlatStep``); ``lr``: float or one-element device tensor; ``step``: one-element
    float32 device tensor counting the steps taken (incremented).  CPU tensors: the same arithmetic with PyTorch ops."""
    if not params.is_cuda:
        t = float(step.item()) + 1.0
        lr_v = float(lr.item()) if torch.is_tensor(lr) else float(lr)
        exp_avg.lerp_(grads, 1.0 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(grads, grads, value=1.0 - beta2)
        denom = (exp_avg_sq.sqrt() / (1.0 - beta2 ** t) ** 0.5).add_(eps)
        params.addcdiv_(exp_avg, denom, value=-lr_v / (1.0 - beta1 ** t))
        step.add_(1.0)
        return
    lr_dev = lr if torch.is_tensor(lr) else None
    rc = _sr().isrAdamFlatStep(_ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), params.numel(), _ptr(lr_dev),
                               0.0 if lr_dev is not None else float(lr), float(beta1), float(beta2), float(eps), _ptr(step), _stream())
    if rc != 0:
        raise RuntimeError("isrAdamFlatStep failed (%d)" % rc)


# ---- fused frame assembly (inference) ---------------------------------------------------------
INIT_MODES = {"zero": 0, "unshaded": 1, "input": 2}


def assemble_input(gbuffer_hwc, flow_filled, prev_high, initial_image="zero", ao_inverted=False, out=None, rows=None, cols=None):
    """Renderer G-buffer [h,w,12] (+ hole-filled flow [1,2,h,w], previous frame [1,6,4h,4w] or None)
    -> network input [1,101,h,w] in one launch (``isrAssembleInput``).  ``rows`` = (row0, row1): only those rows are written
    (``isrAssembleInputRows``; the rest of the result is uninitialised unless ``out`` was given)."""
    assert gbuffer_hwc.is_cuda and gbuffer_hwc.is_contiguous() and gbuffer_hwc.shape[-1] == 12
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    if out is None:
        out = torch.empty((1, 101, h, w), dtype=torch.float32, device=gbuffer_hwc.device)
    elif getattr(out, '_isr_prepacked', None) is not None:
        del out._isr_prepacked                      # a tensor assemble_input_packed handed out before: its planes are written now
    if prev_high is not None:
        prev_high = prev_high.contiguous()
        flow_filled = flow_filled.contiguous()
        assert prev_high.shape == (1, 6, 4 * h, 4 * w) and flow_filled.shape == (1, 2, h, w)
    r0, r1 = (0, h) if rows is None else (int(rows[0]), int(rows[1]))
    c0, c1 = (0, w) if cols is None else (int(cols[0]), int(cols[1]))          # ``cols``: likewise columns (a screen tile + halo)
    rc = _sr().isrAssembleInputRect(_ptr(gbuffer_hwc), _ptr(flow_filled) if prev_high is not None else None,
                                    _ptr(prev_high), _ptr(out), h, w, INIT_MODES[initial_image], 1 if ao_inverted else 0, r0, r1, c0, c1, _stream())
    if rc != 0:
        raise RuntimeError("isrAssembleInput failed (%d)" % rc)
    return out


# the frame's input assembly writes the dataflow trunk's packed-split input itself (isrAssembleInputPacked): one pass over memory and
# one kernel boundary less per frame than assembling fp32 planes and packing them
ASSEMBLE_PACKED = os.environ.get("ISR_ASSEMBLE_PACKED", "1") != "0"


def assemble_input_packed(gbuffer_hwc, flow_filled, prev_high, convs, initial_image="zero", ao_inverted=False):
    """``assemble_input`` for a frame whose trunk runs as the dataflow launch (``convs``: what ``trunk_supported`` takes): the network
    input goes PACKED-SPLIT straight into that launch's workspace.  Returns x [1,101,h,w] of which only channels 0 .. 4 are written
    (what the frame's finishing reads) -- ``x._isr_prepacked`` holds the workspace, ``trunk_dataflow`` then skips its packing pass and
    ``forward_features`` refuses any other route -- or None when the dataflow trunk would not take this frame (assemble the plain way).
    Same values through the same split as the packing pass: the frame is bit-identical."""
    assert gbuffer_hwc.is_cuda and gbuffer_hwc.is_contiguous() and gbuffer_hwc.shape[-1] == 12
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    if not ASSEMBLE_PACKED:
        return None
    out = torch.empty((1, 101, h, w), dtype=torch.float32, device=gbuffer_hwc.device)
    if not trunk_supported(out, convs):
        return None
    if prev_high is not None:
        prev_high = prev_high.contiguous()
        flow_filled = flow_filled.contiguous()
        assert prev_high.shape == (1, 6, 4 * h, 4 * w) and flow_filled.shape == (1, 2, h, w)
    ws = _trunk_workspace(out.device, 101, h, w)
    rc = _sr().isrAssembleInputPacked(_ptr(gbuffer_hwc), _ptr(flow_filled) if prev_high is not None else None, _ptr(prev_high), _ptr(out),
                                      h, w, INIT_MODES[initial_image], 1 if ao_inverted else 0, _ptr(ws), _stream())
    if rc == -3:
        return None
    if rc != 0:
        raise RuntimeError("isrAssembleInputPacked failed (%d)" % rc)
    out._isr_prepacked = ws
    return out


_fill_ws = {}
_FILL_WS_MAX = 16                               # (device, size, stream) workspaces kept; a frame pipeline uses one or two


FLOW_FILL_ONE = os.environ.get("ISR_FLOW_FILL_ONE", "1") != "0"       # the push-pull pyramid as ONE launch (isrFlowFillOne) where it applies


def _fill_failed(st):
    global FLOW_FILL_ONE
    st["buf"][_FILL_ERROR_SLOT] = 0
    FLOW_FILL_ONE = False                       # whoever catches this goes on with the three-launch form
    _routing_changed()                          # a captured frame that holds the one-launch fill is stale (pipeline._graph_signature)
    # A launch that gave up leaves its workspace's ticket / flag words out of step.  The workspaces are NOT freed (a captured graph
    # or a launch still in flight on the render stream may point into them): they are zero-filled again at a quiescent point.
    torch.cuda.synchronize()
    for ws in _fill_ws.values():
        ws.zero_()
    torch.cuda.synchronize()
    raise RuntimeError("flow_fill_one_kernel: a workgroup waited 50 ms for the top of the pyramid in a launch since the last look "
                       "(that frame's filled flow is incomplete; is the device shared?).  The three-launch form is used from now on.")


def fill_flow_gbuffer(gbuffer_hwc, out=None, stream=None, threads=1024, one_launch=None):
    """Hole-filled flow [1,2,h,w] straight from the renderer's G-buffer [h,w,12] (``isrFlowFillOne``: one launch, a workgroup
    per 64 x 64 tile; ``isrFlowFillEx``: three launches, for images of more than 256 tiles or ``one_launch=False`` /
    ISR_FLOW_FILL_ONE=0 -- bit-identical).  ``out`` / ``stream``: caller-owned result tensor and HIP stream (the frame pipeline
    fills the flow of the next frame on its render stream); the pyramid workspace is per (device, size, stream);
    ``threads``: workgroup size of the three-launch form's two grid-wide passes."""
    lib = _sr()
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    st = torch.cuda.current_stream() if stream is None else stream
    key = (gbuffer_hwc.device, h, w, st.cuda_stream)
    ws = _fill_ws.pop(key, None)
    if ws is None:
        if len(_fill_ws) >= _FILL_WS_MAX:
            # bounded: the key holds a raw stream handle (streams come and go in a long-lived viewer).  The least recently used workspace is
            # dropped at a quiescent point -- a launch in flight or a captured frame may still point into it, so: synchronise, and tell the
            # frame pipelines that what they captured is stale
            torch.cuda.synchronize()
            _fill_ws.pop(next(iter(_fill_ws)))
            _routing_changed()
        with torch.cuda.stream(st):             # zero-filled once, in stream order with its first use: the one-launch form's tickets live in it
            ws = torch.zeros(lib.isrFlowFillWorkspace(h, w), dtype=torch.uint8, device=gbuffer_hwc.device)
    _fill_ws[key] = ws                          # (re-inserted: most recently used last)
    if out is None:
        out = torch.empty((1, 2, h, w), dtype=torch.float32, device=gbuffer_hwc.device)
    one = (FLOW_FILL_ONE and not DEVICE_SHARED) if one_launch is None else one_launch
    if one and lib.isrFlowFillOneSupported(h, w):
        # the error word is one of the per-frame guard words whether or not the RANGE guard is on (a spin kernel's timeout must
        # never go to a word that nobody reads)
        lib.isrSetFlowFillErrorWord(ctypes.c_void_p(_range_state(gbuffer_hwc.device)["buf"].data_ptr() + 4 * _FILL_ERROR_SLOT))
        rc = lib.isrFlowFillOne(_ptr(gbuffer_hwc), _ptr(out), _ptr(ws), h, w, ctypes.c_void_p(st.cuda_stream))
    else:
        rc = lib.isrFlowFillEx(_ptr(gbuffer_hwc), _ptr(out), _ptr(ws), h, w, int(threads), ctypes.c_void_p(st.cuda_stream))
    if rc != 0:
        raise RuntimeError("isrFlowFill failed (%d)" % rc)
    return out


def _shading_args(shading):
    """(params[18], specular exponent, ao, inverse_ao, enable_specular) as the finishing kernels take them; ``shading`` None (no rgb
    is asked for): a null ``params`` and the neutral values."""
    if shading is None:
        return None, 1, 0.0, 0, 0
    return ((ctypes.c_float * 18)(*shading.packed_parameters()), int(shading._specular_exponent), float(shading._ao),
            int(bool(shading.inverse_ao)), int(bool(shading.enable_specular)))


def final_conv_finish(features, weight, bias, net_input, shading=None):
    """The network's last layer (64 -> 6, no activation) and ``finish_frame`` in one launch
    (``isrConvSmallFinishFrame``): features [1,Cin,4h,4w] (channel planes may be padded), net_input [1,>=5,h,w]
    -> (next_prev [1,6,4h,4w], rgb [1,3,4h,4w] or None)."""
    assert features.is_cuda and features.shape[0] == 1 and weight.shape[0] == 6
    lib = _sr()
    w8, b8 = _prepare_small(weight, bias)
    features, xp, _ = _plane_strides(features)
    net_input = net_input.contiguous()
    _, cin, H, W = features.shape
    h, w = H // 4, W // 4
    nxt = torch.empty((1, 6, H, W), dtype=torch.float32, device=features.device)
    rgb = torch.empty((1, 3, H, W), dtype=torch.float32, device=features.device) if shading is not None else None
    rc = lib.isrConvSmallFinishFrame(_ptr(features), _ptr(w8), _ptr(b8), _ptr(net_input), _ptr(nxt), _ptr(rgb), cin, h, w, xp,
                                     *_shading_args(shading), _stream())
    if rc != 0:
        raise RuntimeError("isrConvSmallFinishFrame failed (%d)" % rc)
    return nxt, rgb


# ---- the fused 1080p tail (csrc/sr_conv_tail.hip): postblock.6 + postblock.8 + frame finish without the 64-channel round trip ----
TAIL_FUSION = True
_tail_cache = _WeightImages(64)
_tail_ws = {}                    # (device, h, w, stream, output channels) -> workspace of the fused tail


def _prepare_tail(weight8):
    """The last layer's weights [6, 64, 3, 3] (colour networks: [3, 64, 3, 3]) by (tap, channel) row in the z stage's operand order,
    cached like ``prepare_weights``."""
    lib = _sr()

    def build():
        wz = torch.empty(lib.isrConvTailWeightBytes(), dtype=torch.uint8, device=weight8.device)
        prepare = lib.isrConvTailPrepare3 if weight8.shape[0] == 3 else lib.isrConvTailPrepare
        return wz, prepare(_ptr(weight8.detach().contiguous()), _ptr(wz), _stream())
    return _tail_cache.get(id(weight8), (weight8,), build, "isrConvTailPrepare")


def tail_supported(features, weight6, weight8):
    """Can ``tail_conv_finish`` (64 -> 64 -> 6 channels) or ``tail_conv_finish_colour`` (64 -> 64 -> 3) take this frame?  (One image,
    16-byte aligned rows; the default split-operand inference mode.)"""
    if not (TAIL_FUSION and SPLIT_F16 and not FAST_F16 and features.is_cuda and features.dtype == torch.float32):
        return False
    if any_hot(features.device):          # range guard: a layer of this model needs the exact kernels -- per-layer routing only
        return False
    if features.dim() != 4 or features.shape[0] != 1 or features.shape[1] != 64 or features.shape[2] % 4 or features.shape[3] % 4:
        return False
    if tuple(weight6.shape) != (64, 64, 3, 3) or tuple(weight8.shape) not in ((6, 64, 3, 3), (3, 64, 3, 3)):
        return False
    f, xp, _ = _plane_strides(features)
    return f is features and bool(_sr().isrConvTailSupported(_ptr(features), features.shape[2] // 4, features.shape[3] // 4, xp))


class PackedSplit:
    """An activation tensor [1, C, H, W] in PACKED-SPLIT form: every value already split into the (hi, lo') fp16 pair the
    split-operand kernels multiply, eight channels of one pixel per 16-byte unit, ``data[part: hi | lo][C / 8][plane units]``
    (csrc/sr_split_common.h, SplitConvParams::ps).  Produced by ``conv3x3_split_packed``, consumed by ``tail_conv_finish``:
    the consumer stages its k-steps with plain 16-byte copies (LDS-DMA) -- same numbers as converting an fp32 tensor on the
    way in, without the conversions, the staging registers and the producer's LDS transposition."""

    def __init__(self, data, channels, h, w, plane):
        self.data, self.channels, self.h, self.w, self.plane = data, channels, h, w, plane
        self.range_key = None      # range guard: the producer whose flag word describes these values

    @classmethod
    def empty(cls, channels, h, w, device, range_key=None):
        """An uninitialised one for a producer to write (planes padded like the fp32 activations', ``plane_pad``)."""
        plane = h * w + plane_pad(h, w)
        out = cls(torch.empty(2 * (channels // 8) * plane * 4, dtype=torch.int32, device=device), channels, h, w, plane)
        out.range_key = range_key
        return out

    def to_float(self):
        """The fp32 tensor this stands for, hi + lo' 2^-11 (tests)."""
        u = self.data.view(torch.float16).view(2, self.channels // 8, self.plane, 8)[:, :, :self.h * self.w].float()
        v = u[0] + u[1] * (2.0 ** -11)
        return v.permute(0, 2, 1).reshape(1, self.channels, self.h, self.w)


TAIL_PACKED = os.environ.get("ISR_TAIL_PACKED", "1") != "0"       # hand postblock.4's output to the fused tail packed-split (frame pipeline)


def conv3x3_split_packed(x, weight, bias=None, act='relu', slope=0.01, upsample2x=False):
    """``conv3x3_split`` (no autograd, one image, Cout a multiple of 8) whose result is written PACKED-SPLIT."""
    lib = _sr()
    x, xp, _ = _plane_strides(x)
    assert x.shape[0] == 1 and weight.shape[0] % 8 == 0
    cin, cout = weight.shape[1], weight.shape[0]
    h, w = (2 * x.shape[2], 2 * x.shape[3]) if upsample2x else (x.shape[2], x.shape[3])
    if upsample2x and not lib.isrConvF16SupportsUpsample(x.data_ptr(), x.shape[3], xp, cin * xp):
        raise ValueError("conv3x3_split_packed: the fused upsampling needs 16-byte aligned low-resolution rows")
    out = PackedSplit.empty(cout, h, w, x.device, range_key=_arm_range(id(weight), x.device))
    rc = lib.isrConv3x3ForwardSplitPacked(_ptr(x), _ptr(_prepare_split(weight)), _ptr(bias.detach().contiguous() if bias is not None else None),
                                          _ptr(out.data), cin, h, w, cout, ACT_CODES[act], float(slope), 1 if upsample2x else 0, xp, out.plane, _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3ForwardSplitPacked failed (%d)" % rc)
    return out


def conv3x3_split_from_packed(xp, weight, bias=None, act='none', slope=0.01, residual=None, packed_out=False):
    """The split-operand convolution of a PACKED-SPLIT input (``PackedSplit``, staged by LDS-DMA): act(conv3x3(x) + bias)
    + residual as an fp32 tensor, or (``packed_out``, no residual) packed-split again."""
    lib = _sr()
    cout, cin = weight.shape[0], weight.shape[1]
    assert isinstance(xp, PackedSplit) and xp.channels == cin and cin % 8 == 0
    h, w = xp.h, xp.w
    rp = 0
    if residual is not None:
        residual, rp, _ = _plane_strides(residual)
    key = _arm_range(id(weight), xp.data.device)
    if packed_out:
        assert residual is None and cout % 8 == 0
        out = PackedSplit.empty(cout, h, w, xp.data.device, range_key=key)
        y, yplane = out.data, out.plane
    else:
        out = y = empty_planes(1, cout, h, w, xp.data.device)
        out._isr_range_key = key
        yplane = out.stride(1)
    rc = lib.isrConv3x3ForwardSplitFromPacked(_ptr(xp.data), _ptr(_prepare_split(weight)), _ptr(bias.detach().contiguous() if bias is not None else None),
                                              _ptr(residual), _ptr(y), 1 if packed_out else 0, cin, h, w, cout, ACT_CODES[act], float(slope),
                                              xp.plane, yplane, rp, _stream())
    if rc != 0:
        raise RuntimeError("isrConv3x3ForwardSplitFromPacked failed (%d)" % rc)
    return out


# ---- phase-decomposed upsampling layers (csrc/sr_conv_upsp.h): conv3x3(U2(x)) without interpolation at run time ------------------
# U2 (bilinear x2) is linear: the convolution at the high-resolution pixel (2y + py, 2x + px) is a 3 x 3 convolution of the LOW-
# resolution image with one of four effective weight sets.  Input and output are PACKED-SPLIT; the output's one-pixel frame (where the
# convolution's zero padding bites) is computed by a small exact kernel of its own.  Not bit-identical to the interpolate-then-convolve
# kernels (different roundings), the same distance from an fp64 convolution (tests/test_upsp_gpu.py).
# OPT-IN (ISR_UPS_PHASE=1): built, parity-green and MEASURED SLOWER in round 5 -- 1080p layer 0.60 ms + 0.08 ms frame kernel against
# 0.47 ms of conv3x3_split_ups3_kernel.  Why (profiles/r05_upsp_ablation.md): with every operand arriving by LDS-DMA the launch's
# MFMAs + operand reads alone take 0.345 ms at the clock the matrix pipe really holds (~1.5 GHz under load, not the 2.4 GHz the
# roofline's peak is priced at), the operand DMA adds 0.08 ms of LDS write traffic beside 0.67 LDS reads per MFMA, and the four
# epilogues per tile with their stride-2 pixel stores 0.17 ms; the interpolating kernel was never more than 35 % above that floor.
UPS_PHASE = os.environ.get("ISR_UPS_PHASE", "0") == "1"
_upsp_cache = _WeightImages(64)


def _prepare_ups_phase(weight):
    """The stacked image of the four effective weight sets of a [64, 64, 3, 3] weight (``isrConvUpsPhasePrepare``), cached per weight version."""
    lib = _sr()

    def build():
        wq = torch.empty(lib.isrConvUpsPhaseWeightBytes(), dtype=torch.uint8, device=weight.device)
        scratch = torch.empty(lib.isrConvUpsPhaseScratchBytes(), dtype=torch.uint8, device=weight.device)
        return wq, lib.isrConvUpsPhasePrepare(_ptr(weight.detach().contiguous()), _ptr(wq), _ptr(scratch), _stream())
    return _upsp_cache.get(id(weight), (weight,), build, "isrConvUpsPhasePrepare")


def pack_split(x):
    """fp32 [1, C, H, W] -> ``PackedSplit`` (what a producer's packed epilogue would have written; ``isrPackSplit``)."""
    x, xp, _ = _plane_strides(x)
    _, c, h, w = x.shape
    assert x.shape[0] == 1 and c % 8 == 0
    out = PackedSplit.empty(c, h, w, x.device, range_key=getattr(x, '_isr_range_key', None))
    rc = _sr().isrPackSplit(_ptr(x), _ptr(out.data), c, h, w, xp, out.plane, _stream())
    if rc != 0:
        raise RuntimeError("isrPackSplit failed (%d)" % rc)
    return out


def ups_phase_supported(xp, weight):
    """Can ``conv3x3_ups_phase`` take this layer (a 64 -> 64 convolution of the x2-upsampled packed-split tensor ``xp``)?"""
    if not (UPS_PHASE and SPLIT_F16 and not FAST_F16 and isinstance(xp, PackedSplit) and xp.channels == 64 and tuple(weight.shape) == (64, 64, 3, 3)):
        return False
    if any_hot(xp.data.device) or range_is_hot(xp.range_key, xp.data.device):
        return False
    H, W = 2 * xp.h, 2 * xp.w
    return bool(_sr().isrConvUpsPhaseSupported(64, 64, xp.h, xp.w, xp.plane, H * W + plane_pad(H, W)))


def conv3x3_ups_phase(xp, weight, bias=None, act='relu', slope=0.01):
    """act(conv3x3(U2(x), weight) + bias) of a packed-split x [64, h, w] -> packed-split [64, 2h, 2w] (``isrConvUpsPhase``)."""
    lib = _sr()
    assert isinstance(xp, PackedSplit) and xp.channels == 64 and tuple(weight.shape) == (64, 64, 3, 3)
    wq = _prepare_ups_phase(weight)
    out = PackedSplit.empty(64, 2 * xp.h, 2 * xp.w, xp.data.device, range_key=_arm_range(id(weight), xp.data.device))
    rc = lib.isrConvUpsPhase(_ptr(xp.data), _ptr(wq), _ptr(weight.detach().contiguous()), _ptr(bias.detach().contiguous() if bias is not None else None),
                             _ptr(out.data), xp.h, xp.w, ACT_CODES[act], float(slope), xp.plane, out.plane, _stream())
    if rc != 0:
        raise RuntimeError("isrConvUpsPhase failed (%d)" % rc)
    return out


def packed_supported(x, weight, upsample2x):
    """Can ``conv3x3_split_packed`` + the packed tail take this layer?"""
    if not (TAIL_PACKED and x.is_cuda and x.dtype == torch.float32 and x.shape[0] == 1 and weight.shape[0] == 64):
        return False
    if any_hot(x.device):
        return False
    x2, xp, _ = _plane_strides(x)
    if x2 is not x:
        return False
    h, w = (2 * x.shape[2], 2 * x.shape[3]) if upsample2x else (x.shape[2], x.shape[3])
    if h % 4 or w % 4 or 16 * 16 * (h * w + plane_pad(h, w)) >= 2 ** 31:
        return False
    return (not upsample2x) or bool(_sr().isrConvF16SupportsUpsample(x.data_ptr(), x.shape[3], xp, x.shape[1] * xp))


def _tail_operands(features, weight6, bias6, weight8, bias8, net_input, cout):
    """What ``tail_conv_finish`` (``cout`` 6) and ``tail_conv_finish_colour`` (3) do alike, everything up to the output tensors:
    -> (features are packed-split?, device, H, W, plane stride of the features, the library call's seven leading tensors).  Arms
    the range flag: the caller launches next, with nothing but allocations in between."""
    lib = _sr()
    packed = isinstance(features, PackedSplit)
    if packed:
        H, W, xp, dev = features.h, features.w, features.plane, features.data.device
        assert features.channels == 64
        features = features.data
    else:
        features, xp, _ = _plane_strides(features)
        _, _, H, W = features.shape
        dev = features.device
    net_input = net_input.contiguous()
    h, w = H // 4, W // 4
    wq6 = _prepare_split(weight6)
    wz = _prepare_tail(weight8)
    key = (dev, h, w, torch.cuda.current_stream().cuda_stream, cout)
    ws = _tail_ws.get(key)
    if ws is None:
        ws = torch.empty((lib.isrConvTailWorkspaceBytes3 if cout == 3 else lib.isrConvTailWorkspaceBytes)(h, w), dtype=torch.uint8, device=dev)
        _tail_ws[key] = ws
    b6 = bias6.detach().contiguous() if bias6 is not None else None
    b8 = bias8.detach().contiguous() if bias8 is not None else torch.zeros(cout, dtype=torch.float32, device=dev)
    _arm_range(("tail", id(weight6)), dev, members=[id(weight6)])         # the largest |y6|: the intermediate is split in registers inside the kernel
    return packed, dev, H, W, xp, (features, wq6, b6, wz, b8, ws, net_input)


def tail_conv_finish(features, weight6, bias6, weight8, bias8, net_input, shading=None, out=None):
    """features [1,64,4h,4w] (the output of postblock.4; channel planes may be padded) -> relu(conv3x3(., weight6) + bias6)
    -> conv3x3(., weight8) + bias8 -> ``finish_frame``: (next_prev [1,6,4h,4w], rgb [1,3,4h,4w] or None) in two launches
    (``isrConvTailFinishFrame``); the 64-channel tensor between the two convolutions never exists in memory.
    ``out``: (next_prev, rgb) tensors to write into (the frame graph's static output buffers)."""
    lib = _sr()
    packed, dev, H, W, xp, operands = _tail_operands(features, weight6, bias6, weight8, bias8, net_input, 6)
    nxt = out[0] if out is not None else torch.empty((1, 6, H, W), dtype=torch.float32, device=dev)
    assert tuple(nxt.shape) == (1, 6, H, W) and nxt.is_contiguous() and nxt.dtype == torch.float32
    rgb = None
    if shading is not None:
        rgb = out[1] if out is not None else torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        assert tuple(rgb.shape) == (1, 3, H, W) and rgb.is_contiguous()
    fn = lib.isrConvTailFinishFramePacked if packed else lib.isrConvTailFinishFrame
    rc = fn(*map(_ptr, operands), _ptr(nxt), _ptr(rgb), H // 4, W // 4, xp, *_shading_args(shading), _stream())
    if rc != 0:
        raise RuntimeError("isrConvTailFinishFrame failed (%d)" % rc)
    return nxt, rgb


def finish_frame(raw, net_input, shading=None):
    """Conv output before reconstruction [1,6,4h,4w] + network input [1,>=5,h,w] -> (next_prev [1,6,4h,4w],
    rgb [1,3,4h,4w] or None) in one launch (``isrFinishFrame``).  ``shading``: a utils.ScreenSpaceShading."""
    raw = raw.contiguous()
    net_input = net_input.contiguous()
    _, _, H, W = raw.shape
    h, w = H // 4, W // 4
    nxt = torch.empty_like(raw)
    rgb = torch.empty((1, 3, H, W), dtype=torch.float32, device=raw.device) if shading is not None else None
    rc = _sr().isrFinishFrame(_ptr(raw), _ptr(net_input), _ptr(nxt), _ptr(rgb), h, w, *_shading_args(shading), _stream())
    if rc != 0:
        raise RuntimeError("isrFinishFrame failed (%d)" % rc)
    return nxt, rgb


# ---- colour networks (RGB in, RGB out; inference.LoadedModel with ``unshaded == False``) -------------------------------------------
# The two ends of the frame that depend on what the network is for: the input assembly (channel selection + warp and space-to-depth of
# the previous RGB frame) and the finishing (residual reconstruction over [0, 1, 2] + clamp), standalone, behind the small-Cout last
# layer, and behind the fused tail with three output channels.  One [1, 3, 4h, 4w] tensor is the displayed RGB and the next ``prev_high``.
COLOUR_VARIANTS = (8, 7, 5, 4)          # number of selected G-buffer channels: normal + depth, normal, depth, neither


def assemble_input_colour(gbuffer_hwc, flow_filled, prev_high, variant, initial_image="zero", out=None):
    """Renderer G-buffer [h,w,12] (+ hole-filled flow [1,2,h,w], previous frame [1,3,4h,4w] or None) -> the colour network's input
    [1, variant + 48, h, w] in one launch (``isrAssembleInputColour``).  ``variant``: 8 | 7 | 5 | 4 selected channels
    (``LoadedModel.input_single_channels`` + 3 for normal + 1 for depth).  Without a previous frame ``initial_image`` "zero" needs no
    flow; "input" (the x4 bilinear RGB, warped like any previous frame) does; "unshaded" raises ValueError as ``utils.initialImage``."""
    assert gbuffer_hwc.is_cuda and gbuffer_hwc.is_contiguous() and gbuffer_hwc.shape[-1] == 12
    if variant not in COLOUR_VARIANTS:
        raise ValueError("assemble_input_colour: variant must be one of %s" % (COLOUR_VARIANTS,))
    if prev_high is None and initial_image == "unshaded":
        raise ValueError("for mode='unshaded', channels is expected to be 5 or 6")
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    if out is None:
        out = torch.empty((1, variant + 48, h, w), dtype=torch.float32, device=gbuffer_hwc.device)
    assert tuple(out.shape) == (1, variant + 48, h, w) and out.is_contiguous()
    need_flow = prev_high is not None or initial_image == "input"
    if need_flow:
        if flow_filled is None:
            raise ValueError("assemble_input_colour: the hole-filled flow is needed (a previous frame, or initial image 'input')")
        flow_filled = flow_filled.contiguous()
        assert flow_filled.shape == (1, 2, h, w)
    if prev_high is not None:
        prev_high = prev_high.contiguous()
        assert prev_high.shape == (1, 3, 4 * h, 4 * w)
    rc = _sr().isrAssembleInputColour(_ptr(gbuffer_hwc), _ptr(flow_filled) if need_flow else None, _ptr(prev_high), _ptr(out), h, w,
                                      int(variant), INIT_MODES[initial_image] if prev_high is None else 0, _stream())
    if rc != 0:
        raise RuntimeError("isrAssembleInputColour failed (%d)" % rc)
    return out


def finish_frame_colour(raw, net_input):
    """Conv output before reconstruction [1,3,4h,4w] + network input [1,>=3,h,w] -> clamp(raw + bilinear x4 of net_input[:, :3], 0, 1)
    in one launch (``isrFinishFrameColour``): ``clamp(ops.recon_residual(raw, net_input, 3), 0, 1)`` bit for bit."""
    raw = raw.contiguous()
    net_input = net_input.contiguous()
    assert raw.is_cuda and raw.shape[0] == 1 and raw.shape[1] == 3 and net_input.shape[1] >= 3
    _, _, H, W = raw.shape
    out = torch.empty_like(raw)
    rc = _sr().isrFinishFrameColour(_ptr(raw), _ptr(net_input), _ptr(out), H // 4, W // 4, _stream())
    if rc != 0:
        raise RuntimeError("isrFinishFrameColour failed (%d)" % rc)
    return out


def final_conv_finish_colour(features, weight, bias, net_input):
    """The colour network's last layer (64 -> 3, the exact small-Cout kernel) and ``finish_frame_colour`` in one launch
    (``isrConvSmallFinishFrameColour``) -- the route of frames whose layers the range guard has sent to the exact kernels."""
    assert features.is_cuda and features.shape[0] == 1 and weight.shape[0] == 3
    w8, b8 = _prepare_small(weight, bias)
    features, xp, _ = _plane_strides(features)
    net_input = net_input.contiguous()
    _, cin, H, W = features.shape
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=features.device)
    rc = _sr().isrConvSmallFinishFrameColour(_ptr(features), _ptr(w8), _ptr(b8), _ptr(net_input), _ptr(out), cin, H // 4, W // 4, xp, _stream())
    if rc != 0:
        raise RuntimeError("isrConvSmallFinishFrameColour failed (%d)" % rc)
    return out


def tail_conv_finish_colour(features, weight6, bias6, weight8, bias8, net_input, out=None):
    """``tail_conv_finish`` for a colour network: features [1,64,4h,4w] (fp32, or a ``PackedSplit``) -> relu(conv3x3(., weight6) +
    bias6) -> conv3x3(., weight8 [3,64,3,3]) + bias8 -> ``finish_frame_colour``, in two launches (``isrConvTailFinishFrame3``): nine
    S planes and 27 rows of the extra product instead of eighteen and 54.  Returns [1,3,4h,4w] (``out`` to write into)."""
    lib = _sr()
    assert tuple(weight8.shape) == (3, 64, 3, 3) and net_input.shape[1] >= 3
    packed, dev, H, W, xp, operands = _tail_operands(features, weight6, bias6, weight8, bias8, net_input, 3)
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    assert tuple(out.shape) == (1, 3, H, W) and out.is_contiguous() and out.dtype == torch.float32
    fn = lib.isrConvTailFinishFrame3Packed if packed else lib.isrConvTailFinishFrame3
    rc = fn(*map(_ptr, operands), _ptr(out), H // 4, W // 4, xp, _stream())
    if rc != 0:
        raise RuntimeError("isrConvTailFinishFrame3 failed (%d)" % rc)
    return out


# ---- RCAN: channel attention and the pixel-shuffle tail (csrc/sr_attention.hip) -------------------------------------------------------------
# The three pieces of models/rcan.py that are not convolutions.  Each function's CPU branch is its DEFINITION in plain torch (as
# ``conv3x3``'s is); a device tensor without autograd takes the HIP kernels where ``*_supported`` says so and the same torch composite
# (with a warning, once) where the kernels refuse.  Under autograd ``channel_attention_residual`` (without ``return_gate``) and
# ``pixel_shuffle4_conv`` are ONE autograd node each on the same forward kernels -- the result has the bits of the no-grad call -- with their
# own backward kernels (``_ChannelAttentionFunction``: at most three launches, ``_PixelShuffle4ConvFunction``: three) where
# ``*_backward_supported`` says so, and the torch composite, silently, where it does not (CPU, fp64, other shapes, a library without the
# backward entry points, ``return_gate``).  ``channel_pool`` on its own is the torch composite under autograd: nothing trains through it alone.
ATTENTION_CHANNELS = 64
ATTENTION_REDUCED = 4
# False: the three ops run their torch composite on the device without a word (tools/bench_rcan.py's comparison: the same network with
# its non-convolution pieces on PyTorch-ROCm's operators).  A MEASUREMENT switch: the composite's output is not watched by the range guard.
ATTENTION_KERNELS = True


def _any_requires_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _strides_of(t):
    """(plane, image) strides ``_plane_strides`` will hand to a kernel for ``t`` -- without copying anything."""
    n, c, h, w = t.shape
    if t.stride(3) == 1 and t.stride(2) == w and t.stride(1) >= h * w and (n == 1 or t.stride(0) >= c * t.stride(1)):
        return t.stride(1), t.stride(0) if n > 1 else c * t.stride(1)
    return h * w, c * h * w


def channel_pool_supported(t):
    """``isrChannelPool`` takes this tensor: fp32 [N, 64, H, W] on the device, one image below 2 GiB."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.numel() > 0):
        return False
    n, c, h, w = t.shape
    plane, image = _strides_of(t)
    return bool(_sr().isrChannelPoolSupported(n, c, h, w, plane, image))


def _channel_pool_cpu(t):
    n, c, h, w = t.shape
    return torch.mean(t.reshape(n, c, h * w), dim=2)


def _pool_partials(t):
    """-> (t with packed rows, plane stride, image stride, S, workspace double [N][64][S]) after ``isrChannelPool``."""
    lib = _sr()
    t, tp, ti = _plane_strides(t)
    n, c, h, w = t.shape
    slabs = lib.isrChannelPoolSlabs(n, h, w)
    ws = torch.empty(n * c * slabs, dtype=torch.float64, device=t.device)
    rc = lib.isrChannelPool(_ptr(t), tp, ti, n, c, h, w, slabs, _ptr(ws), _stream())
    if rc != 0:
        raise RuntimeError("isrChannelPool failed (%d)" % rc)
    return t, tp, ti, slabs, ws


def channel_pool(t):
    """[N, 64, H, W] -> the [N, 64] mean over H x W (the squeeze of the channel attention).  HIP: slab sums in fp64 in a fixed order
    (``isrChannelPool``), summed in index order and rounded to fp32 once (``isrChannelPoolMean``): two calls give the same bits."""
    if not t.is_cuda or _any_requires_grad(t) or not ATTENTION_KERNELS:
        return _channel_pool_cpu(t)
    if not channel_pool_supported(t):
        _warn_once("channel_pool", "channel_pool: %s is not what the HIP kernel takes; torch.mean runs instead" % (tuple(t.shape),))
        return _channel_pool_cpu(t)
    with torch.no_grad():
        t, _, _, slabs, ws = _pool_partials(t)
        n, c, h, w = t.shape
        mean = torch.empty((n, c), dtype=torch.float32, device=t.device)
        rc = _sr().isrChannelPoolMean(_ptr(ws), n, c, h, w, slabs, _ptr(mean), _stream())
        if rc != 0:
            raise RuntimeError("isrChannelPoolMean failed (%d)" % rc)
        return mean


def channel_attention_supported(x, t, w_down, w_up):
    """The two attention launches take these operands: x, t fp32 [N, 64, H, W] on one device, a 64 -> 4 -> 64 perceptron."""
    if not (channel_pool_supported(t) and channel_pool_supported(x) and x.shape == t.shape and x.device == t.device):
        return False
    n, c, h, w = x.shape
    if not all(_sr().isrChannelGateScaleAddSupported(n, c, w_down.shape[0], h, w, *_strides_of(v)) for v in (x, t)):
        return False
    return tuple(w_down.shape) == (ATTENTION_REDUCED, ATTENTION_CHANNELS) and tuple(w_up.shape) == (ATTENTION_CHANNELS, ATTENTION_REDUCED) \
        and w_down.dtype == torch.float32 and w_up.dtype == torch.float32 and w_down.is_cuda and w_up.is_cuda


def _channel_attention_cpu(x, t, w_down, b_down, w_up, b_up, slope, return_gate):
    z = _channel_pool_cpu(t)
    s = torch.sigmoid(F.linear(F.leaky_relu(F.linear(z, w_down, b_down), slope), w_up, b_up))
    y = x + t * s[:, :, None, None]
    return (y, s) if return_gate else y


def channel_attention_residual(x, t, w_down, b_down, w_up, b_up, slope=0.01, return_gate=False, range_key=None):
    """A residual channel-attention block's ``x + t * s``: s [N, 64] = sigmoid(W_up leaky_relu(W_down mean_hw(t) + b_down) + b_up)
    (``nn.Linear`` layouts).  HIP: two launches -- ``isrChannelPool`` and ``isrChannelGateScaleAdd`` (the perceptron recomputed per
    workgroup in a fixed fmaf order; given s, y is bitwise ``x + t * s[:, :, None, None]``).  ``return_gate``: -> (y, s).
    ``range_key``: the range guard's word this launch reports the largest |y| to (``_arm_range``; models/rcan.py hands in the word of
    the block's second convolution, so that a block costs one word): y is tagged with it, and a hot y sends its consumer to the exact
    kernels through ``conv3x3``'s routing; without a key y counts as of unknown range only if x or t do."""
    if (x.is_cuda and ATTENTION_KERNELS and not return_gate and _any_requires_grad(x, t, w_down, b_down, w_up, b_up)
            and channel_attention_backward_supported(x, t, w_down, b_down, w_up, b_up)):
        return _ChannelAttentionFunction.apply(x, t, w_down, b_down, w_up, b_up, float(slope))
    if not x.is_cuda or _any_requires_grad(x, t, w_down, b_down, w_up, b_up) or not ATTENTION_KERNELS:
        return _channel_attention_cpu(x, t, w_down, b_down, w_up, b_up, slope, return_gate)
    if not channel_attention_supported(x, t, w_down, w_up):
        _warn_once("channel_attention", "channel_attention_residual: %s is not what the HIP kernels take; PyTorch operators run instead"
                   % (tuple(x.shape),))
        out = _channel_attention_cpu(x, t, w_down, b_down, w_up, b_up, slope, return_gate)
        (out[0] if return_gate else out)._isr_range_key = HOT          # nobody watched its range
        return out
    with torch.no_grad():
        unknown = HOT in (getattr(x, '_isr_range_key', None), getattr(t, '_isr_range_key', None))
        y, gate, key = _attention_forward(x, t, w_down, b_down, w_up, b_up, slope, return_gate, range_key)[:3]
        y._isr_range_key = HOT if unknown else key
        return (y, gate) if return_gate else y


def _attention_forward(x, t, w_down, b_down, w_up, b_up, slope, want_gate, range_key, packed=False):
    """The two forward launches -> (y, gate [N, 64] or None, the armed range word or None, t as the kernels read it, S, the pool's
    workspace).  ``packed``: y is an ordinary contiguous tensor (the autograd node's output), else ``empty_planes``."""
    lib = _sr()
    t, tp, ti, slabs, ws = _pool_partials(t)
    x, xp, xi = _plane_strides(x)
    n, c, h, w = x.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device) if packed else empty_planes(n, c, h, w, x.device)
    gate = torch.empty((n, c), dtype=torch.float32, device=x.device) if want_gate else None
    wd, bd, wu, bu = (p.detach().contiguous() for p in (w_down, b_down, w_up, b_up))
    key = _arm_range(range_key, x.device) if range_key is not None else None
    rc = lib.isrChannelGateScaleAdd(_ptr(x), _ptr(t), _ptr(y), xp, xi, tp, ti, y.stride(1), c * y.stride(1), _ptr(ws), slabs,
                                    _ptr(wd), _ptr(bd), _ptr(wu), _ptr(bu), float(slope), _ptr(gate), n, c, ATTENTION_REDUCED, h, w, _stream())
    if rc != 0:
        raise RuntimeError("isrChannelGateScaleAdd failed (%d)" % rc)
    return y, gate, key, t, slabs, ws


def channel_attention_backward_supported(x, t, w_down, b_down, w_up, b_up):
    """``_ChannelAttentionFunction`` takes these operands: what the forward kernels take, fp32 biases on the device, and a library that
    has the backward entry points."""
    lib = _sr()
    if not hasattr(lib, "isrChannelGateScaleBackward") or not channel_attention_supported(x, t, w_down, w_up):
        return False
    if not all(b.is_cuda and b.dtype == torch.float32 for b in (b_down, b_up)):
        return False
    n, c, h, w = t.shape
    return all(lib.isrChannelAttentionBackwardSupported(n, c, ATTENTION_REDUCED, h, w, *s) for s in (_strides_of(t), (h * w, c * h * w)))


class _ChannelAttentionFunction(torch.autograd.Function):
    """y = x + t * s as ONE autograd node.  Forward: the two launches of the no-grad route (no range word armed: the training rule of
    ``_train_conv``) and ``isrChannelPoolMean``; t, the mean z and the gate s are saved.  Backward: dx IS dy; ``isrChannelGateGradSums``
    (ds = sum_hw dy t), ``isrChannelGateScaleBackward`` (dt, only if t needs a gradient) and ``isrChannelGateParamGrad`` (only if a
    parameter of the perceptron does) -- nothing is launched when neither does."""

    @staticmethod
    def forward(ctx, x, t, w_down, b_down, w_up, b_up, slope):
        y, gate, _, t, slabs, ws = _attention_forward(x, t, w_down, b_down, w_up, b_up, slope, True, None, packed=True)
        n, c, h, w = t.shape
        mean = torch.empty((n, c), dtype=torch.float32, device=t.device)
        rc = _sr().isrChannelPoolMean(_ptr(ws), n, c, h, w, slabs, _ptr(mean), _stream())
        if rc != 0:
            raise RuntimeError("isrChannelPoolMean failed (%d)" % rc)
        ctx.slope = slope
        ctx.save_for_backward(t, mean, gate, w_down, b_down, w_up)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        t, mean, gate, w_down, b_down, w_up = ctx.saved_tensors
        need = ctx.needs_input_grad
        gx = gy if need[0] else None
        if not any(need[1:6]):
            return gx, None, None, None, None, None, None
        lib = _sr()
        n, c, h, w = t.shape
        t, tp, ti = _plane_strides(t)
        g, gp, gi = _plane_strides(gy)
        if not lib.isrChannelAttentionBackwardSupported(n, c, ATTENTION_REDUCED, h, w, gp, gi):
            g, gp, gi = gy.contiguous(), h * w, c * h * w
        slabs = lib.isrChannelPoolSlabs(n, h, w)
        ws = torch.empty(n * c * slabs, dtype=torch.float64, device=t.device)
        rc = lib.isrChannelGateGradSums(_ptr(g), gp, gi, _ptr(t), tp, ti, n, c, h, w, slabs, _ptr(ws), _stream())
        if rc != 0:
            raise RuntimeError("isrChannelGateGradSums failed (%d)" % rc)
        wd, bd, wu = (p.detach().contiguous() for p in (w_down, b_down, w_up))
        dt = dwd = dbd = dwu = dbu = None
        if need[1]:
            dt = torch.empty((n, c, h, w), dtype=torch.float32, device=t.device)
            rc = lib.isrChannelGateScaleBackward(_ptr(g), gp, gi, _ptr(dt), h * w, c * h * w, _ptr(ws), slabs, _ptr(mean), _ptr(gate),
                                                 _ptr(wd), _ptr(bd), _ptr(wu), ctx.slope, n, c, ATTENTION_REDUCED, h, w, _stream())
            if rc != 0:
                raise RuntimeError("isrChannelGateScaleBackward failed (%d)" % rc)
        if any(need[2:6]):
            dwd, dbd, dwu, dbu = (torch.empty(s, dtype=torch.float32, device=t.device)
                                  for s in ((ATTENTION_REDUCED, c), (ATTENTION_REDUCED,), (c, ATTENTION_REDUCED), (c,)))
            rc = lib.isrChannelGateParamGrad(_ptr(ws), slabs, _ptr(mean), _ptr(gate), _ptr(wd), _ptr(bd), _ptr(wu), ctx.slope,
                                             _ptr(dwd), _ptr(dbd), _ptr(dwu), _ptr(dbu), n, c, ATTENTION_REDUCED, h, w, _stream())
            if rc != 0:
                raise RuntimeError("isrChannelGateParamGrad failed (%d)" % rc)
        return (gx, dt, dwd if need[2] else None, dbd if need[3] else None, dwu if need[4] else None, dbu if need[5] else None, None)


def pixel_shuffle4_conv_supported(f, weight):
    """``isrShuffleTailColour`` takes these operands: f fp32 [N, 64, h, w] on the device, weight [Cout <= 8, 4, 3, 3]."""
    if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.float32 and f.dim() == 4 and f.numel() > 0 and weight.is_cuda
            and weight.dtype == torch.float32 and weight.dim() == 4 and tuple(weight.shape[1:]) == (4, 3, 3)):
        return False
    n, c, h, w = f.shape
    plane, image = _strides_of(f)
    cout = weight.shape[0]
    return bool(_sr().isrShuffleTailColourSupported(n, c, cout, h, w, plane, image, 16 * h * w, cout * 16 * h * w))


def _pixel_shuffle4_conv_cpu(f, weight, bias, clamp):
    out = F.conv2d(F.pixel_shuffle(f, 4), weight, bias, padding=1)
    return torch.clamp(out, 0, 1) if clamp else out


def pixel_shuffle4_conv(f, weight, bias, clamp=False):
    """RCAN's tail: conv3x3(pixel_shuffle(f [N, 64, h, w], 4), weight [Cout, 4, 3, 3], padding 1) + bias -> [N, Cout, 4h, 4w], clamped
    to [0, 1] with ``clamp``.  HIP: one launch (``isrShuffleTailColour``), the shuffled four-channel tensor stays in LDS; per value an
    fp32 fmaf chain over (ci, ky, kx) starting from the bias.  Under autograd: the same launch as one autograd node
    (``_PixelShuffle4ConvFunction``; ``clamp`` is then ``torch.clamp`` behind it -- the same bits), or ``F.pixel_shuffle`` and
    ``F.conv2d`` where ``pixel_shuffle4_conv_backward_supported`` says no."""
    if f.is_cuda and ATTENTION_KERNELS and _any_requires_grad(f, weight, bias) and pixel_shuffle4_conv_backward_supported(f, weight, bias):
        out = _PixelShuffle4ConvFunction.apply(f, weight, bias)
        return torch.clamp(out, 0, 1) if clamp else out
    if not f.is_cuda or _any_requires_grad(f, weight, bias) or not ATTENTION_KERNELS:
        return _pixel_shuffle4_conv_cpu(f, weight, bias, clamp)
    if not pixel_shuffle4_conv_supported(f, weight):
        _warn_once("pixel_shuffle4_conv", "pixel_shuffle4_conv: %s with weight %s is not what the HIP kernel takes; PyTorch operators run instead"
                   % (tuple(f.shape), tuple(weight.shape)))
        return _pixel_shuffle4_conv_cpu(f, weight, bias, clamp)
    with torch.no_grad():
        return _tail_forward(f, weight, bias, clamp)[0]


def _tail_forward(f, weight, bias, clamp):
    """The forward launch -> (out, f as the kernel read it)."""
    f, fp, fi = _plane_strides(f)
    n, c, h, w = f.shape
    cout = weight.shape[0]
    out = torch.empty((n, cout, 4 * h, 4 * w), dtype=torch.float32, device=f.device)
    wt = weight.detach().contiguous()
    b = bias.detach().contiguous() if bias is not None else None
    rc = _sr().isrShuffleTailColour(_ptr(f), fp, fi, _ptr(wt), _ptr(b), _ptr(out), 16 * h * w, cout * 16 * h * w, n, c, cout, h, w,
                                    1 if clamp else 0, _stream())
    if rc != 0:
        raise RuntimeError("isrShuffleTailColour failed (%d)" % rc)
    return out, f


def pixel_shuffle4_conv_backward_supported(f, weight, bias):
    """``_PixelShuffle4ConvFunction`` takes these operands: what the forward kernel takes, an fp32 bias on the device (or none), and a
    library that has the backward entry points."""
    lib = _sr()
    if not hasattr(lib, "isrShuffleTailDataGrad") or not pixel_shuffle4_conv_supported(f, weight):
        return False
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32):
        return False
    n, c, h, w = f.shape
    cout = weight.shape[0]
    return all(lib.isrShuffleTailBackwardSupported(n, c, cout, h, w, *s, 16 * h * w, cout * 16 * h * w) for s in (_strides_of(f), (h * w, c * h * w)))


class _PixelShuffle4ConvFunction(torch.autograd.Function):
    """out = conv3x3(pixel_shuffle(f, 4), w) + b as ONE autograd node: forward ``isrShuffleTailColour``; backward
    ``isrShuffleTailDataGrad`` (one launch, only if f needs a gradient) and ``isrShuffleTailWeightGrad`` (two launches, only if the
    weight or the bias does)."""

    @staticmethod
    def forward(ctx, f, weight, bias):
        out, f = _tail_forward(f, weight, bias, False)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(f, weight)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        f, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        lib = _sr()
        n, c, h, w = f.shape
        cout = weight.shape[0]
        f, fp, fi = _plane_strides(f)
        g = g.contiguous()
        gp, gi = 16 * h * w, cout * 16 * h * w
        df = dw = db = None
        if need[0]:
            df = torch.empty((n, c, h, w), dtype=torch.float32, device=f.device)
            rc = lib.isrShuffleTailDataGrad(_ptr(g), gp, gi, _ptr(weight.detach().contiguous()), _ptr(df), h * w, c * h * w, n, c, cout, h, w, _stream())
            if rc != 0:
                raise RuntimeError("isrShuffleTailDataGrad failed (%d)" % rc)
        if need[1] or (ctx.has_bias and need[2]):
            tiles = lib.isrShuffleTailGradTiles(n, h, w)
            ws = torch.empty(tiles * cout * 37, dtype=torch.float64, device=f.device)
            dw = torch.empty((cout, 4, 3, 3), dtype=torch.float32, device=f.device)
            db = torch.empty(cout, dtype=torch.float32, device=f.device) if ctx.has_bias else None
            rc = lib.isrShuffleTailWeightGrad(_ptr(g), gp, gi, _ptr(f), fp, fi, n, c, cout, h, w, tiles, _ptr(ws), _ptr(dw), _ptr(db), _stream())
            if rc != 0:
                raise RuntimeError("isrShuffleTailWeightGrad failed (%d)" % rc)
        return df, dw if need[1] else None, db if (ctx.has_bias and need[2]) else None


# ---- batch normalisation of the EnhanceNet blocks (models/enhancenet.py with use_bn; csrc/sr_batchnorm.hip) ---------------------------
# Two halves.  In eval mode a layer is an affine map per channel: ``fold_batch_norm`` folds it into the convolution in front of it and
# the network IS a plain EnhanceNet -- every fused route applies, nothing new is launched.  In training mode ``batch_norm`` is ONE
# autograd node on the kernels of csrc/sr_batchnorm.hip: three launches forward (slab sums, the once-only finishing step, the streaming
# pass), three backward; sums in fp64 in a fixed order, so a call repeats bit for bit; no host read, so the call can be captured.
# False: ``batch_norm`` is the ``nn.BatchNorm2d`` module itself on the device without a word (tools/bench_bn_train.py's comparison and the
# tests' A/B).  A MEASUREMENT switch.
BATCH_NORM_KERNELS = True
_fold_cache = weakref.WeakKeyDictionary()          # bn module -> [weakref(conv weight), stamps of the six sources, epoch, weight', bias']


def _bn_shape_ok(x, bn):
    return torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == bn.num_features and x.numel() > 0


def batch_norm_supported(x, bn):
    """Does ``batch_norm(x, bn)`` run the HIP kernels?  A training-mode ``nn.BatchNorm2d`` with a fixed momentum, affine parameters and
    running statistics, all fp32 on the device of the fp32 tensor x [N, C, H, W] with N H W >= 2.  Everything else -- the CPU, eval
    mode, ``momentum=None``, ``affine=False``, ``track_running_stats=False``, another dtype -- is the ``F.batch_norm`` composition."""
    if not (BATCH_NORM_KERNELS and bn.training and _bn_shape_ok(x, bn) and x.is_cuda and x.dtype == torch.float32):
        return False
    if bn.momentum is None or not bn.affine or not bn.track_running_stats or bn.running_mean is None:
        return False
    if not all(t.dtype == torch.float32 and t.device == x.device and t.is_contiguous() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)):
        return False
    n, c, h, w = x.shape
    lib = _sr()
    return hasattr(lib, "isrBatchNormStats") and bool(lib.isrBatchNormSupported(n, c, h, w))


def _batch_norm_torch(x, bn, act, residual):
    # nn.BatchNorm2d.forward: F.batch_norm and the bookkeeping around it.  On the device ATen's own kernels, not the vendor library's:
    # that one takes the variance in one fp32 pass and is 1.5e-5 of max|y| off where a channel's mean is large against its spread
    # (tests/test_bn_gpu.py), ATen's (Welford) stay within the bars of the HIP kernels.
    vendor = torch.backends.cudnn.enabled
    if x.is_cuda:
        torch.backends.cudnn.enabled = False
    try:
        y = bn(x)
    finally:
        torch.backends.cudnn.enabled = vendor
    if act == 'relu':
        y = F.relu(y)
    return y + residual if residual is not None else y


def _batch_norm_forward(x, bn, weight, bias, relu, residual):
    """The three forward launches -> (y, x as the kernels read it, mean, invstd); the running statistics are updated in place."""
    lib = _sr()
    x = x.contiguous()
    n, c, h, w = x.shape
    res = residual.contiguous() if residual is not None else None
    slabs = lib.isrBatchNormSlabs(n, c, h, w)
    ws = torch.empty(2 * c * n * slabs, dtype=torch.float64, device=x.device)
    mean, invstd = torch.empty((2, c), dtype=torch.float32, device=x.device).unbind(0)
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    rc = lib.isrBatchNormStats(_ptr(x), n, c, h, w, slabs, _ptr(ws), float(bn.eps), float(bn.momentum), _ptr(mean), _ptr(invstd),
                               _ptr(bn.running_mean), _ptr(bn.running_var), _stream())
    if rc != 0:
        raise RuntimeError("isrBatchNormStats failed (%d)" % rc)
    # (the kernel wrote the two buffers through their addresses: their version counters say so to whoever keys on them -- fold_batch_norm)
    torch.autograd.graph.increment_version(bn.running_mean)
    torch.autograd.graph.increment_version(bn.running_var)
    rc = lib.isrBatchNormApply(_ptr(x), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), _ptr(res), 1 if relu else 0, _ptr(y), n, c, h, w,
                               _stream())
    if rc != 0:
        raise RuntimeError("isrBatchNormApply failed (%d)" % rc)
    return y, x, mean, invstd


class _BatchNormFunction(torch.autograd.Function):
    """act(batch_norm(x)) + residual as ONE autograd node: the three forward launches of the no-grad route; x, mean, invstd (and y for
    the ReLU form, whose sign gates dy) are saved.  Backward: ``isrBatchNormGradSums`` (two launches: slab sums, then dgamma, dbeta and
    the streaming pass's coefficients), ``isrBatchNormBackward`` only if x needs a gradient; the residual's gradient IS dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, bn, relu):
        y, x, mean, invstd = _batch_norm_forward(x, bn, weight, bias, relu, residual)
        ctx.relu = relu
        ctx.save_for_backward(x, y if relu else None, mean, invstd, weight)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, y, mean, invstd, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        gres = gy if need[3] else None
        if not any(need[0:3]):
            return None, None, None, gres, None, None
        lib = _sr()
        n, c, h, w = x.shape
        g = gy.contiguous()
        slabs = lib.isrBatchNormSlabs(n, c, h, w)
        ws = torch.empty(2 * c * n * slabs, dtype=torch.float64, device=x.device)
        coef = torch.empty(2 * c, dtype=torch.float32, device=x.device)
        dgamma = torch.empty(c, dtype=torch.float32, device=x.device) if need[1] else None
        dbeta = torch.empty(c, dtype=torch.float32, device=x.device) if need[2] else None
        rc = lib.isrBatchNormGradSums(_ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), n, c, h, w, slabs, _ptr(ws), _ptr(coef),
                                      _ptr(dgamma), _ptr(dbeta), _stream())
        if rc != 0:
            raise RuntimeError("isrBatchNormGradSums failed (%d)" % rc)
        dx = None
        if need[0]:
            dx = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
            rc = lib.isrBatchNormBackward(_ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(coef), _ptr(dx), n, c, h, w,
                                          _stream())
            if rc != 0:
                raise RuntimeError("isrBatchNormBackward failed (%d)" % rc)
        return dx, dgamma, dbeta, gres, None, None


def batch_norm(x, bn, act='none', residual=None):
    """``act(bn(x)) + residual`` for an ``nn.BatchNorm2d`` -- the two combinations of an EnhanceNet block: act='relu' without a residual
    (the first layer of a block), no activation plus the block's skip (the second).  A training-mode layer on the device: the kernels
    of csrc/sr_batchnorm.hip (``batch_norm_supported``), forward-only under ``no_grad``; batch statistics with the biased variance, the
    running statistics updated once, in place, with the unbiased one, ``num_batches_tracked += 1`` as the torch op it is.  On the CPU
    the ``F.batch_norm`` composition IS the definition; on the device it is what runs -- after a warning, once -- where the kernels do
    not apply.  One value per channel in training mode raises ``ValueError``, as PyTorch does."""
    if act not in ('none', 'relu'):
        raise ValueError("batch_norm: unknown activation %r" % (act,))
    if act == 'relu' and residual is not None:
        raise ValueError("batch_norm: an activation together with a residual is not a combination of the blocks")
    if not _bn_shape_ok(x, bn):
        raise ValueError("batch_norm: expected a [N, %d, H, W] tensor, got %s" % (bn.num_features, tuple(x.shape)))
    if bn.training and x.numel() // x.shape[1] < 2:
        raise ValueError("batch_norm: expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
    if not x.is_cuda or not BATCH_NORM_KERNELS:
        return _batch_norm_torch(x, bn, act, residual)
    if not batch_norm_supported(x, bn):
        _warn_once("batch_norm", "batch_norm: the HIP kernels take a training-mode fp32 layer with momentum, affine parameters and running "
                   "statistics; F.batch_norm runs instead (%s, training=%s)" % (tuple(x.shape), bn.training))
        return _batch_norm_torch(x, bn, act, residual)
    if residual is not None and (residual.shape != x.shape or residual.dtype != torch.float32 or residual.device != x.device):
        raise ValueError("batch_norm: the residual must be an fp32 tensor of x's shape on x's device")
    if _any_requires_grad(x, bn.weight, bn.bias, residual):
        y = _BatchNormFunction.apply(x, bn.weight, bn.bias, residual, bn, act == 'relu')
    else:
        with torch.no_grad():
            y = _batch_norm_forward(x, bn, bn.weight, bn.bias, act == 'relu', residual)[0]
            y._isr_range_key = HOT                   # nobody watched its range: its consumer takes the exact kernels
    if bn.num_batches_tracked is not None:
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
    return y


def _fold_sources(weight, bias, bn):
    return (weight, bias, bn.weight, bn.bias, bn.running_mean, bn.running_var)


def fold_batch_norm(weight, bias, bn):
    """The convolution an eval-mode ``bn`` behind conv(weight, bias) amounts to -> (weight', bias'), computed in fp64 on the tensors'
    device and rounded to fp32 once: s = gamma / sqrt(running_var + eps), weight' = weight * s[co], bias' = (bias - running_mean) * s
    + beta.  The results are PERSISTENT tensors per layer, rewritten IN PLACE when a source changes, so every image cache downstream
    (``_wcache``, the split images, the dataflow trunk's table) sees an ordinary weight that was updated.  Staleness is the rule of
    ``_WeightImages``: the (_version, data_ptr) of each of the six sources and ``_images_epoch`` -- a graph replay moves the running
    statistics without advancing ``_version``, and ``train.GraphedTrainStep`` calls ``invalidate_weight_images()`` after each."""
    if bn.running_mean is None or bn.running_var is None:
        raise ValueError("fold_batch_norm: the layer tracks no running statistics; there is nothing to fold")
    sources = _fold_sources(weight, bias, bn)
    stamp = _WeightImages._stamp(sources)
    hit = _fold_cache.get(bn)
    if hit is not None and hit[0]() is weight and hit[1] == stamp and hit[2] == _images_epoch:
        return hit[3], hit[4]
    with torch.no_grad():
        var = bn.running_var.detach().double()
        s = torch.rsqrt(var + bn.eps) if bn.weight is None else bn.weight.detach().double() / torch.sqrt(var + bn.eps)
        w = (weight.detach().double() * s[:, None, None, None]).float()
        b = -bn.running_mean.detach().double() if bias is None else bias.detach().double() - bn.running_mean.detach().double()
        b = b * s
        if bn.bias is not None:
            b = b + bn.bias.detach().double()
        b = b.float()
        if hit is not None and hit[0]() is weight and hit[3].shape == w.shape and hit[3].device == w.device:
            hit[3].copy_(w); hit[4].copy_(b)          # in place: the tensors' _version moves, their consumers' images follow
            hit[1], hit[2] = stamp, _images_epoch
            return hit[3], hit[4]
    _fold_cache[bn] = [weakref.ref(weight), stamp, _images_epoch, w, b]
    return w, b


# ---- training batches from device-resident clips (dataset_video.DeviceClips; csrc/sr_dataset.hip) --------------------------------------
# ``clips``: an object with the flat fp32 buffers ``high``, ``low``, ``flow`` (every clip [T, Ch, r H, r W] / [T, Cl, H, W] / [T, 2, H, W],
# one after the other), ``table`` (int64 [clips, 5]: the clip's element offset in each of the three, H, W), ``frames``,
# ``low_channels``, ``high_channels``, ``upscale`` and ``high_quad_aligned`` (every high offset a multiple of four elements).
# ``samples``: int32 [n, 4] -- clip, first row x0, first column y0 of the low-resolution crop, augmentation mode 0..3.
_SHADED_LOW_CHANNELS = (7, 8)                      # layouts with a normal at channels 4, 5 (dataset_video.data_augmentation)


def _clip_sign_masks(low_channels):
    """(low, flow) x (row flip, column flip): bit ch set = the flip negates channel ch."""
    shaded = low_channels in _SHADED_LOW_CHANNELS
    return (1 << 4 if shaded else 0, 1 << 5 if shaded else 0), (1 << 0, 1 << 1)


def _gather_operands(clips, samples, indices, crop):
    buffers = (clips.high, clips.low, clips.flow)
    if any(t.dtype != torch.float32 for t in buffers):
        raise ValueError("gather_clips: the clip buffers must be fp32, got %s" % ([str(t.dtype) for t in buffers],))
    if clips.table.dtype != torch.int64 or samples.dtype != torch.int32 or indices.dtype != torch.int64:
        raise ValueError("gather_clips: the clip table and the indices are int64, the sample table is int32")
    devices = {t.device for t in buffers + (clips.table, samples, indices)}
    if len(devices) != 1:
        raise ValueError("gather_clips: operands on more than one device: %s" % sorted(str(d) for d in devices))
    if samples.dim() != 2 or samples.shape[1] != 4 or samples.shape[0] < 1 or indices.dim() != 1 or clips.table.dim() != 2 or clips.table.shape[1] != 5:
        raise ValueError("gather_clips: expected samples [n >= 1, 4], indices [B] and a clip table [clips, 5]")
    if int(crop) < 1:
        raise ValueError("gather_clips: crop must be positive")


def gather_clips_supported(clips, samples, indices, crop):
    """Does ``gather_clips`` run the HIP kernel?  Device operands, a library that has the entry point and a batch it takes."""
    if not (clips.high.is_cuda and all(t.is_contiguous() for t in (clips.high, clips.low, clips.flow, clips.table, samples, indices))):
        return False
    lib = _sr()
    return hasattr(lib, "isrClipGather") and bool(lib.isrClipGatherSupported(indices.shape[0], clips.frames, clips.low_channels,
                                                                             clips.high_channels, int(crop), clips.upscale))


def _gather_clips_torch(clips, samples, indices, crop, augment):
    # THE DEFINITION: DatasetFromSamples.__getitem__ + data_augmentation + the default collate, on the flat buffers
    T, r = clips.frames, clips.upscale
    rows = samples[indices.clamp(0, samples.shape[0] - 1)].tolist()
    table = clips.table.tolist()
    (low_x, low_y), (flow_x, flow_y) = _clip_sign_masks(clips.low_channels)
    parts = ([], [], [])
    for clip, x0, y0, mode in rows:
        off_high, off_low, off_flow, H, W = table[clip]
        flip_x, flip_y = bool(augment and mode & 1), bool(augment and mode & 2)
        dims = [d for d, f in ((2, flip_x), (3, flip_y)) if f]
        for out, buf, off, C, s, neg_x, neg_y in ((parts[0], clips.low, off_low, clips.low_channels, 1, low_x, low_y),
                                                  (parts[1], clips.flow, off_flow, 2, 1, flow_x, flow_y),
                                                  (parts[2], clips.high, off_high, clips.high_channels, r, 0, 0)):
            t = buf[off:off + T * C * s * H * s * W].view(T, C, s * H, s * W)[:, :, s * x0:s * (x0 + crop), s * y0:s * (y0 + crop)]
            t = t.flip(dims) if dims else t.clone()
            for ch in range(C):
                if flip_x and (neg_x >> ch) & 1: t[:, ch] = -t[:, ch]
                if flip_y and (neg_y >> ch) & 1: t[:, ch] = -t[:, ch]
            out.append(t)
    hr = r * crop
    shapes = ((0, T, clips.low_channels, crop, crop), (0, T, 2, crop, crop), (0, T, clips.high_channels, hr, hr))
    return tuple(torch.stack(p) if p else torch.empty(sh, dtype=torch.float32, device=clips.high.device) for p, sh in zip(parts, shapes))


def gather_clips(clips, samples, indices, crop, augment=False):
    """The training batch ``(input [B, T, Cl, c, c], flow [B, T, 2, c, c], target [B, T, Ch, r c, r c])`` of the samples ``indices``
    (int64 [B]) of device-resident clips: per sample the crop ``[x0:x0 + c, y0:y0 + c]`` of low and flow and r times that box of high,
    all T frames; with ``augment`` mode bit 0 reverses the rows and bit 1 the columns, and the flips negate flow channel 0 / 1 and, in the
    shaded layouts (7 or 8 low channels), low channel 4 / 5 -- ``DatasetFromSamples.__getitem__`` + ``data_augmentation`` + the default
    collate, bit for bit (-0.0 where a zero is negated).  An index outside [0, n - 1] is clamped.  Device operands: ONE launch of
    ``clip_gather_kernel`` on the current stream into fresh tensors, no host read.  CPU operands: the definition in plain torch.  A
    device whose library lacks the entry point runs the definition too -- after a warning, once."""
    _gather_operands(clips, samples, indices, crop)
    crop = int(crop)
    if not clips.high.is_cuda:
        return _gather_clips_torch(clips, samples, indices, crop, augment)
    B = indices.shape[0]
    if B == 0 or not gather_clips_supported(clips, samples, indices, crop):
        if B:
            _warn_once("gather_clips", "gather_clips: the loaded library has no isrClipGather for this batch (%d samples, crop %d); the "
                       "PyTorch definition runs instead, sample by sample" % (B, crop))
        return _gather_clips_torch(clips, samples, indices, crop, augment)
    lib = _sr()
    T, Cl, Ch, r = clips.frames, clips.low_channels, clips.high_channels, clips.upscale
    dev = clips.high.device
    inp = torch.empty((B, T, Cl, crop, crop), dtype=torch.float32, device=dev)
    flow = torch.empty((B, T, 2, crop, crop), dtype=torch.float32, device=dev)
    target = torch.empty((B, T, Ch, r * crop, r * crop), dtype=torch.float32, device=dev)
    (low_x, low_y), (flow_x, flow_y) = _clip_sign_masks(Cl)
    with torch.cuda.device(dev):
        rc = lib.isrClipGather(_ptr(clips.high), _ptr(clips.low), _ptr(clips.flow), _ptr(clips.table), _ptr(samples), samples.shape[0],
                               _ptr(indices), B, T, Cl, Ch, crop, r, 1 if augment else 0, low_x, low_y, flow_x, flow_y,
                               1 if clips.high_quad_aligned else 0, _ptr(inp), _ptr(flow), _ptr(target), _stream())
    if rc != 0:
        raise RuntimeError("isrClipGather failed (%d)" % rc)
    return inp, flow, target


# ---- the clip generator's device side (datagen.py; csrc/sr_dataset.hip) --------------------------------------------------------------
PACK_HIGH_CHANNELS = (3, 4, 5, 6, 7, 10)           # mask (from alpha), normal, depth, ambient occlusion of a G-buffer pixel
PACK_LOW_CHANNELS = (3, 4, 5, 6, 7)


def _pack_operands(low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf, offsets):
    tensors = (low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf)
    if any(t.dtype != torch.float32 for t in tensors):
        raise ValueError("pack_clip_frame: every operand is fp32, got %s" % ([str(t.dtype) for t in tensors],))
    if len({t.device for t in tensors}) != 1:
        raise ValueError("pack_clip_frame: operands on more than one device")
    if low_gbuf.dim() != 3 or low_gbuf.shape[2] != 12 or high_gbuf.dim() != 3 or high_gbuf.shape[2] != 12 or min(low_gbuf.shape) < 1:
        raise ValueError("pack_clip_frame: the G-buffers are [h, w, 12] and [r h, r w, 12], got %s and %s" % (tuple(low_gbuf.shape), tuple(high_gbuf.shape)))
    h, w = int(low_gbuf.shape[0]), int(low_gbuf.shape[1])
    r = int(high_gbuf.shape[0]) // h
    if r < 1 or tuple(high_gbuf.shape[:2]) != (r * h, r * w) or flow.numel() != 2 * h * w or tuple(flow.shape[-2:]) != (h, w):
        raise ValueError("pack_clip_frame: low %s, high %s and flow %s are not [h, w, 12], [r h, r w, 12] and [2, h, w]"
                         % (tuple(low_gbuf.shape), tuple(high_gbuf.shape), tuple(flow.shape)))
    n = h * w
    for name, buf, off, size in zip(("high", "low", "flow"), (high_buf, low_buf, flow_buf), offsets,
                                    (len(PACK_HIGH_CHANNELS) * r * r * n, len(PACK_LOW_CHANNELS) * n, 2 * n)):
        if buf.dim() != 1 or not buf.is_contiguous() or not 0 <= int(off) <= buf.numel() - size:
            raise ValueError("pack_clip_frame: %d elements at offset %d do not fit the flat %s buffer of %s" % (size, off, name, tuple(buf.shape)))
    return h, w, r


def pack_clip_frame_supported(low_gbuf, high_gbuf, flow):
    """Does ``pack_clip_frame`` run the HIP kernel?  Contiguous device operands, 16-byte aligned G-buffers, a library that has the entry
    point and a frame it takes."""
    if not (low_gbuf.is_cuda and all(t.is_contiguous() for t in (low_gbuf, high_gbuf, flow))) or low_gbuf.data_ptr() % 16 or high_gbuf.data_ptr() % 16:
        return False
    lib = _sr()
    return hasattr(lib, "isrClipPackFrame") and bool(lib.isrClipPackFrameSupported(low_gbuf.shape[0], low_gbuf.shape[1],
                                                                                   high_gbuf.shape[0] // low_gbuf.shape[0]))


def _pack_clip_frame_torch(low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf, offsets):
    # THE DEFINITION: convertToNumpy of DataGenerator/DataGeneratorVideo2.py:66-77 on G-buffers instead of EXR files.  Only the alpha is
    # clipped (torch.clamp keeps a NaN, as np.clip does); normals, depth and AO are copied.
    for gbuf, channels, buf, off in ((high_gbuf, PACK_HIGH_CHANNELS, high_buf, int(offsets[0])), (low_gbuf, PACK_LOW_CHANNELS, low_buf, int(offsets[1]))):
        planes = gbuf.permute(2, 0, 1)[list(channels)].clone()
        planes[0] = planes[0].clamp(0, 1) * 2 - 1
        buf[off:off + planes.numel()].copy_(planes.reshape(-1))
    flow_buf[int(offsets[2]):int(offsets[2]) + flow.numel()].copy_(flow.reshape(-1))


def pack_clip_frame(low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf, offsets):
    """One frame of a training clip from its two renders: the G-buffers ``low_gbuf`` [h, w, 12] and ``high_gbuf`` [r h, r w, 12] and the
    hole-filled ``flow`` [2, h, w] (or [1, 2, h, w]) into the flat fp32 buffers at the element ``offsets`` (high, low, flow) -- six planes
    ``[clamp(g[3], 0, 1) 2 - 1, g[4], g[5], g[6], g[7], g[10]]`` of the high render, five ``[clamp(g[3], 0, 1) 2 - 1, g[4..7]]`` of the low
    one, the flow copied: the reference's ``convertToNumpy``.  Device operands: ONE launch of ``clip_pack_kernel`` on the current stream,
    no host read.  CPU operands: the definition in plain torch.  A device whose library lacks the entry point, or operands the kernel
    does not take, run the definition too -- after a warning, once."""
    _pack_operands(low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf, offsets)
    if low_gbuf.is_cuda and pack_clip_frame_supported(low_gbuf, high_gbuf, flow):
        h, w = low_gbuf.shape[0], low_gbuf.shape[1]
        with torch.cuda.device(low_gbuf.device):
            rc = _sr().isrClipPackFrame(_ptr(low_gbuf), _ptr(high_gbuf), _ptr(flow), h, w, high_gbuf.shape[0] // h, _ptr(high_buf), int(offsets[0]),
                                        _ptr(low_buf), int(offsets[1]), _ptr(flow_buf), int(offsets[2]), _stream())
        if rc != 0:
            raise RuntimeError("isrClipPackFrame failed (%d)" % rc)
        return
    if low_gbuf.is_cuda:
        _warn_once("pack_clip_frame", "pack_clip_frame: the loaded library has no isrClipPackFrame for these operands (low %s); the PyTorch "
                   "definition runs instead" % (tuple(low_gbuf.shape),))
    _pack_clip_frame_torch(low_gbuf, high_gbuf, flow, high_buf, low_buf, flow_buf, offsets)


def coverage_table_offsets(rows):
    """Element offset of every clip's pair of tables in the flat result of ``clip_coverage``, and its length: ``rows`` is the clip
    table as a list; clip k takes 2 (H + 1) (W + 1) elements."""
    offsets, total = [], 0
    for row in rows:
        offsets.append(total)
        total += 2 * (int(row[3]) + 1) * (int(row[4]) + 1)
    return offsets, total


def _clip_coverage_torch(low_buf, rows, frames, low_channels, out, offsets):
    # THE DEFINITION: the summed-area table of dataset_video.collect_samples' coverage indicator, (c0 + c1) + c2 > 0 in fp32
    for (_, off_low, _, H, W), start in zip(rows, offsets):
        clip = low_buf[off_low:off_low + frames * low_channels * H * W].view(frames, low_channels, H, W)
        for k, t in enumerate((0, frames - 1)):
            covered = ((clip[t, 0] + clip[t, 1]) + clip[t, 2]) > 0
            sat = torch.zeros((H + 1, W + 1), dtype=torch.int32, device=low_buf.device)
            sat[1:, 1:] = covered.to(torch.int64).cumsum(0).cumsum(1).to(torch.int32)
            at = start + k * (H + 1) * (W + 1)
            out[at:at + sat.numel()].copy_(sat.reshape(-1))


def clip_coverage(low_buf, table, frames, low_channels=5, rows=None):
    """Summed-area tables of the crop-coverage indicator ``low[0] + low[1] + low[2] > 0`` of the first and the last frame of every clip
    in the flat buffer ``low_buf``: a flat int32 tensor holding ``[2, H + 1, W + 1]`` per clip, one after the other
    (``coverage_table_offsets``; a tensor ``[clips, 2, H + 1, W + 1]`` where the clips have one size).  ``table``: the int64 [clips, 5]
    clip table on ``low_buf``'s device; ``rows``: its host copy where the caller has one (otherwise it is read back).  Device operands:
    ONE launch of ``clip_coverage_kernel``, a workgroup per table.  CPU operands: the definition (``cumsum``)."""
    if low_buf.dtype != torch.float32 or low_buf.dim() != 1 or table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 5:
        raise ValueError("clip_coverage: a flat fp32 buffer and an int64 clip table [clips, 5]")
    if table.device != low_buf.device or frames < 1 or low_channels < 3:
        raise ValueError("clip_coverage: table on %s, buffer on %s, %d frames, %d channels" % (table.device, low_buf.device, frames, low_channels))
    rows = [tuple(int(v) for v in row) for row in (table.tolist() if rows is None else rows)]
    for k, (_, off_low, _, H, W) in enumerate(rows):
        if H < 1 or W < 1 or not 0 <= off_low <= low_buf.numel() - frames * low_channels * H * W:
            raise ValueError("clip_coverage: clip %d (%d x %d at %d) leaves the buffer of %d elements" % (k, H, W, off_low, low_buf.numel()))
    offsets, total = coverage_table_offsets(rows)
    out = torch.empty(total, dtype=torch.int32, device=low_buf.device)
    lib = _sr() if low_buf.is_cuda else None
    if lib is not None and hasattr(lib, "isrClipCoverage") and lib.isrClipCoverageSupported(len(rows), frames, low_channels) \
            and low_buf.is_contiguous() and table.is_contiguous():
        where = torch.tensor(offsets, dtype=torch.int64).to(low_buf.device)
        with torch.cuda.device(low_buf.device):
            rc = lib.isrClipCoverage(_ptr(low_buf), _ptr(table), _ptr(where), len(rows), frames, low_channels, _ptr(out), _stream())
        if rc != 0:
            raise RuntimeError("isrClipCoverage failed (%d)" % rc)
    else:
        if low_buf.is_cuda:
            _warn_once("clip_coverage", "clip_coverage: the loaded library has no isrClipCoverage for %d clips; the PyTorch definition runs instead" % len(rows))
        _clip_coverage_torch(low_buf, rows, frames, low_channels, out, offsets)
    if len({(row[3], row[4]) for row in rows}) == 1:
        out = out.view(len(rows), 2, rows[0][3] + 1, rows[0][4] + 1)
    return out


# ---- the viewer's display stage (viewer.py) --------------------------------------------------------------------------------------------
DISPLAY_VIEWS ={"color": 0, "mask": 1, "normal": 2, "depth": 3, "ao": 4, "flow": 5}       # ISR_VIEW_*


def display_supported(gbuffer_hwc, rgb, raw=None):
    """Can ``display_frame`` take these tensors: fp32 on the device, a [h,w,12] G-buffer, rgb [1,3,4h,4w], raw None or [1,6,4h,4w]?"""
    if not (gbuffer_hwc.is_cuda and rgb.is_cuda and gbuffer_hwc.dtype == torch.float32 and rgb.dtype == torch.float32):
        return False
    if gbuffer_hwc.dim() != 3 or gbuffer_hwc.shape[-1] != 12 or not gbuffer_hwc.is_contiguous():
        return False
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    if not (0 < h <= 16383 and 0 < w <= 16383) or tuple(rgb.shape) != (1, 3, 4 * h, 4 * w):
        return False
    return raw is None or (raw.is_cuda and raw.dtype == torch.float32 and tuple(raw.shape) == (1, 6, 4 * h, 4 * w))


def display_frame(gbuffer_hwc, rgb, raw=None, filled_flow=None, shading=None, channel="color", masking=False, background0=1.0, focus=None,
                  focus_gbuffer=None, bounds=None, prev_displayed=None, post_smoothing=0.0, out=None, out8=None):
    """``viewer.compose_display`` in one launch (``isrDisplayFrame``): same arguments, device tensors; -> ``out`` [1,3,4h,4w] (allocated
    if None; must not be ``prev_displayed``).  ``out8``: a [4h,4w,4] uint8 tensor that receives the RGBA copy.  ``bounds``: the two-float
    device tensor of ``viewer.depth_bounds`` (depth view).  No fall-back: tensors the launch does not take raise."""
    if channel not in DISPLAY_VIEWS:
        raise ValueError("channel must be one of %s" % (tuple(DISPLAY_VIEWS),))
    if not display_supported(gbuffer_hwc, rgb, raw):
        raise ValueError("display_frame: fp32 device tensors gbuffer [h,w,12], rgb [1,3,4h,4w], raw None or [1,6,4h,4w] are needed")
    h, w = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    H, W = 4 * h, 4 * w
    dev = gbuffer_hwc.device
    keep = [rgb.contiguous(), raw.contiguous() if raw is not None else None]
    p = _DisplayParams()
    p.gbuffer, p.rgb, p.raw = gbuffer_hwc.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr() if raw is not None else None
    smoothing = prev_displayed is not None and post_smoothing != 0
    if channel == "flow" or smoothing:
        if filled_flow is None or tuple(filled_flow.shape) != (1, 2, h, w) or not filled_flow.is_cuda or filled_flow.dtype != torch.float32:
            raise ValueError("display_frame: the hole-filled flow [1,2,h,w] is needed (flow view, post-smoothing)")
        keep.append(filled_flow.contiguous())
        p.flow = keep[-1].data_ptr()
    if smoothing:
        if tuple(prev_displayed.shape) != (1, 3, H, W) or not prev_displayed.is_cuda or prev_displayed.dtype != torch.float32:
            raise ValueError("display_frame: prev_displayed must be [1,3,4h,4w] fp32 on the device")
        keep.append(prev_displayed.contiguous())
        p.prev = keep[-1].data_ptr()
        p.smooth_prev = float(np.float32(post_smoothing))
        p.smooth_cur = float(np.float32(1.0 - post_smoothing))
    if focus is not None:
        viewport, mask = focus
        if focus_gbuffer is None or tuple(focus_gbuffer.shape) != (H, W, 12) or not focus_gbuffer.is_cuda or not focus_gbuffer.is_contiguous() \
                or focus_gbuffer.dtype != torch.float32 or shading is None:
            raise ValueError("display_frame: focus needs the full-resolution G-buffer [4h,4w,12] on the device and the shading")
        if mask.numel() != H * W or not mask.is_cuda or mask.dtype != torch.float32:
            raise ValueError("display_frame: the focus mask must be [1,4h,4w] fp32 on the device")
        keep.append(mask.contiguous())
        p.focus, p.focus_mask = focus_gbuffer.data_ptr(), keep[-1].data_ptr()
        x0, y0, x1, y1 = (int(v) for v in viewport)
        p.viewport = (ctypes.c_int * 4)(max(0, x0), max(0, y0), min(W, x1), min(H, y1))
        p.shading = (ctypes.c_float * 18)(*shading.packed_parameters())
        p.exponent, p.ao_strength, p.enable_specular = int(shading._specular_exponent), float(shading._ao), int(bool(shading.enable_specular))
    if channel == "depth":
        if bounds is None:
            d = gbuffer_hwc[..., 7]
            bounds = torch.stack([(d + (d <= 1e-5).to(d.dtype)).min(), d.max()])
        if bounds.numel() != 2 or not bounds.is_cuda or bounds.dtype != torch.float32:
            raise ValueError("display_frame: bounds must be two fp32 values on the device")
        keep.append(bounds.contiguous())
        p.depth_bounds = keep[-1].data_ptr()
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (1, 3, H, W) or not out.is_cuda or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("display_frame: out must be a contiguous [1,3,4h,4w] fp32 device tensor")
    if smoothing and out.data_ptr() == p.prev:
        raise ValueError("display_frame: out must not be prev_displayed (the warp reads neighbouring pixels)")
    p.out = out.data_ptr()
    if out8 is not None:
        if tuple(out8.shape) != (H, W, 4) or not out8.is_cuda or not out8.is_contiguous() or out8.dtype != torch.uint8:
            raise ValueError("display_frame: out8 must be a contiguous [4h,4w,4] uint8 device tensor")
        p.out8 = out8.data_ptr()
    p.h, p.w, p.channel, p.masking, p.background0 = h, w, DISPLAY_VIEWS[channel], int(bool(masking)), float(background0)
    rc = _sr().isrDisplayFrame(ctypes.byref(p), _stream())
    if rc != 0:
        raise RuntimeError("isrDisplayFrame failed (%d)" % rc)
    return out


BASELINE_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2, "ground_truth": 3}           # ISR_BASE_* (ground truth: IDENTITY)


def display_baseline_frame(gbuffer_hwc, mode, shading=None, filled_flow=None, channel="color", focus=None, focus_gbuffer=None, bounds=None,
                           prev_displayed=None, post_smoothing=0.0, out=None, out8=None, workspace=None):
    """``viewer.compose_baseline`` on device tensors (``isrDisplayBaselineFrame``): same arguments; -> ``out`` [1,3,4h,4w] (allocated if
    None; must not be ``prev_displayed``), ``out8`` as ``display_frame``.  ``nearest`` / ``bilinear`` / ``bicubic``: gbuffer [h,w,12],
    two launches (a low-resolution pre-pass into ``workspace``, [12,h,w] fp32, allocated if None; then the display launch);
    ``ground_truth``: gbuffer [4h,4w,12], one launch, focus and post-smoothing are not applied and the flow view raises, as in the
    definition.  ``shading`` is needed by the colour view and by a focus window.  No fall-back: tensors the launch does not take raise."""
    if mode not in BASELINE_MODES:
        raise ValueError("mode must be one of %s" % (tuple(BASELINE_MODES),))
    if channel not in DISPLAY_VIEWS:
        raise ValueError("channel must be one of %s" % (tuple(DISPLAY_VIEWS),))
    truth = mode == "ground_truth"
    if truth:
        if channel == "flow":
            raise ValueError("display_baseline_frame: no flow view in ground-truth mode")
        focus = focus_gbuffer = prev_displayed = None
    if not (torch.is_tensor(gbuffer_hwc) and gbuffer_hwc.is_cuda and gbuffer_hwc.dtype == torch.float32 and gbuffer_hwc.dim() == 3
            and gbuffer_hwc.shape[-1] == 12 and gbuffer_hwc.is_contiguous()):
        raise ValueError("display_baseline_frame: a contiguous fp32 device G-buffer [rows,cols,12] is needed")
    rows, cols = gbuffer_hwc.shape[0], gbuffer_hwc.shape[1]
    if truth and (rows % 4 or cols % 4):
        raise ValueError("display_baseline_frame: the ground-truth G-buffer is [4h,4w,12]")
    h, w = (rows // 4, cols // 4) if truth else (rows, cols)
    if not (0 < h <= 16383 and 0 < w <= 16383):
        raise ValueError("display_baseline_frame: 0 < h, w <= 16383")
    H, W = 4 * h, 4 * w
    dev = gbuffer_hwc.device
    keep = []
    p = _DisplayBaselineParams()
    p.gbuffer = gbuffer_hwc.data_ptr()
    smoothing = prev_displayed is not None and post_smoothing != 0
    if channel == "flow" or smoothing:
        if filled_flow is None or tuple(filled_flow.shape) != (1, 2, h, w) or not filled_flow.is_cuda or filled_flow.dtype != torch.float32:
            raise ValueError("display_baseline_frame: the hole-filled flow [1,2,h,w] is needed (flow view, post-smoothing)")
        keep.append(filled_flow.contiguous())
        p.flow = keep[-1].data_ptr()
    if smoothing:
        if tuple(prev_displayed.shape) != (1, 3, H, W) or not prev_displayed.is_cuda or prev_displayed.dtype != torch.float32:
            raise ValueError("display_baseline_frame: prev_displayed must be [1,3,4h,4w] fp32 on the device")
        keep.append(prev_displayed.contiguous())
        p.prev = keep[-1].data_ptr()
        p.smooth_prev = float(np.float32(post_smoothing))
        p.smooth_cur = float(np.float32(1.0 - post_smoothing))
    if focus is not None:
        viewport, mask = focus
        if focus_gbuffer is None or tuple(focus_gbuffer.shape) != (H, W, 12) or not focus_gbuffer.is_cuda or not focus_gbuffer.is_contiguous() \
                or focus_gbuffer.dtype != torch.float32:
            raise ValueError("display_baseline_frame: focus needs the full-resolution G-buffer [4h,4w,12] on the device")
        if mask.numel() != H * W or not mask.is_cuda or mask.dtype != torch.float32:
            raise ValueError("display_baseline_frame: the focus mask must be [1,4h,4w] fp32 on the device")
        keep.append(mask.contiguous())
        p.focus, p.focus_mask = focus_gbuffer.data_ptr(), keep[-1].data_ptr()
        x0, y0, x1, y1 = (int(v) for v in viewport)
        p.viewport = (ctypes.c_int * 4)(max(0, x0), max(0, y0), min(W, x1), min(H, y1))
    if channel == "color":
        if shading is None:
            raise ValueError("display_baseline_frame: the colour view needs the shading")
        p.shading = (ctypes.c_float * 18)(*shading.packed_parameters())
        p.exponent, p.ao_strength, p.enable_specular = int(shading._specular_exponent), float(shading._ao), int(bool(shading.enable_specular))
    if channel == "depth":
        if bounds is None:
            d = gbuffer_hwc[..., 7]
            bounds = torch.stack([(d + (d <= 1e-5).to(d.dtype)).min(), d.max()])
        if bounds.numel() != 2 or not bounds.is_cuda or bounds.dtype != torch.float32:
            raise ValueError("display_baseline_frame: bounds must be two fp32 values on the device")
        keep.append(bounds.contiguous())
        p.depth_bounds = keep[-1].data_ptr()
    if not truth and channel != "flow":
        if workspace is None:
            workspace = torch.empty((12, h, w), dtype=torch.float32, device=dev)
        if tuple(workspace.shape) != (12, h, w) or not workspace.is_cuda or not workspace.is_contiguous() or workspace.dtype != torch.float32:
            raise ValueError("display_baseline_frame: workspace must be a contiguous [12,h,w] fp32 device tensor")
        p.low_planes = workspace.data_ptr()
    if out is None:
        out = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
    if tuple(out.shape) != (1, 3, H, W) or not out.is_cuda or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("display_baseline_frame: out must be a contiguous [1,3,4h,4w] fp32 device tensor")
    if smoothing and out.data_ptr() == p.prev:
        raise ValueError("display_baseline_frame: out must not be prev_displayed (the warp reads neighbouring pixels)")
    p.out = out.data_ptr()
    if out8 is not None:
        if tuple(out8.shape) != (H, W, 4) or not out8.is_cuda or not out8.is_contiguous() or out8.dtype != torch.uint8:
            raise ValueError("display_baseline_frame: out8 must be a contiguous [4h,4w,4] uint8 device tensor")
        p.out8 = out8.data_ptr()
    p.h, p.w, p.mode, p.channel = h, w, BASELINE_MODES[mode], DISPLAY_VIEWS[channel]
    rc = _sr().isrDisplayBaselineFrame(ctypes.byref(p), _stream())
    if rc != 0:
        raise RuntimeError("isrDisplayBaselineFrame failed (%d)" % rc)
    return out


# ---- the metric stage of the statistics harness (csrc/sr_metrics.hip; stats.Statistics(metrics="hip")) ----

METRICS_SQERR_WORKSPACE_BYTES = 16384           # ISR_METRICS_SQERR_WORKSPACE_BYTES
MSSSIM_LEVELS = 5
MSSSIM_WINDOW = 11


def _image3(t):
    """[C,H,W] view of an image given as [C,H,W] or [1,C,H,W]; None if it is neither."""
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    return t if t.dim() == 3 else None


def _plane2(t, h, w):
    """[H,W] view of a mask / blend plane given as [H,W], [1,H,W] or [1,1,H,W]: fp64 on the device, rows dense."""
    while t.dim() > 2 and t.shape[0] == 1:
        t = t[0]
    if not (t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (h, w) and t.stride(1) == 1 and t.stride(0) >= w):
        raise ValueError("metrics: the mask / blend plane must be a float64 device tensor [%d, %d] with dense rows" % (h, w))
    return t


def metrics_supported(*tensors):
    """Can the metric kernels read these images where they lie: fp32 on one device, [C,H,W] or [1,C,H,W] of one shape, dense rows
    (cropped views are fine: row and plane pitches are passed), non-negative pitches?"""
    first = None
    for t in tensors:
        v = _image3(t) if isinstance(t, torch.Tensor) else None
        if v is None or not v.is_cuda or v.dtype != torch.float32 or v.numel() == 0:
            return False
        c, h, w = v.shape
        if v.stride(2) != 1 or v.stride(1) < w or v.stride(0) < (1 if c > 1 else 0) or c > 64 or h > 32768 or w > 32768:
            return False
        if first is None:
            first = v
        elif v.shape != first.shape or v.device != first.device:
            return False
    return first is not None


def _metric_pair(name, a, b):
    if not metrics_supported(a, b):
        raise ValueError("%s: two float32 device images [C,H,W] of one shape with dense rows are needed" % name)
    a, b = _image3(a), _image3(b)
    return a, b, (_ptr(a), a.stride(1), a.stride(0), _ptr(b), b.stride(1), b.stride(0))


def masked_sq_err(a, b, mask=None):
    """-> float64 device tensor [2]: sum((m a - m b)^2) over the image and sum(m) over its pixels (``utils/psnr.py:12-13``; without a
    mask m = 1).  Two launches on the current stream, nothing synchronises; ``psnr_from_sq_err`` turns it into the PSNR."""
    a, b, views = _metric_pair("masked_sq_err", a, b)
    c, h, w = a.shape
    m = _plane2(mask, h, w) if mask is not None else None
    workspace = torch.empty(METRICS_SQERR_WORKSPACE_BYTES // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(2, dtype=torch.float64, device=a.device)
    rc = _sr().isrMetricsSqErr(*views, _ptr(m), m.stride(0) if m is not None else 0, c, h, w, _ptr(workspace), _ptr(out), _stream())
    if rc != 0:
        raise RuntimeError("isrMetricsSqErr failed (%d)" % rc)
    return out


def psnr_from_sq_err(sq_err, channels, height, width, masked, epsilon=1e-7):
    """``utils.PSNR`` from the two sums of ``masked_sq_err``, on the device (a 0-dim float64 tensor)."""
    mse = sq_err[0] / float(channels * height * width)
    if not masked:
        return 10 * torch.log10(1 / (epsilon + mse))
    return 10 * ((height * width) / sq_err[1]) * torch.log10(1 / (epsilon + mse))          # (the operation order of utils/psnr.py:12-14)


def msssim_windows(height, width, device):
    """float64 [5, 121]: row l holds the k x k table of ``utils.ssim.create_window(k)`` (fp32 products, widened) for MS-SSIM level l of
    an image of this size, k = min(11, H >> l, W >> l).  Depends on the size only: a caller with many frames keeps it."""
    from .utils.ssim import create_window
    table = torch.zeros(MSSSIM_LEVELS, MSSSIM_WINDOW * MSSSIM_WINDOW, dtype=torch.float64)
    for level in range(MSSSIM_LEVELS):
        k = min(MSSSIM_WINDOW, height >> level, width >> level)
        table[level, :k * k] = create_window(k)[0, 0].double().reshape(-1)
    return table.to(device)


def msssim_terms(a, b, blend=None, windows=None):
    """-> float64 device tensor [11]: the mean SSIM map of the five levels, the mean v1 / v2 of the five levels, and their combination
    ``utils.ssim.msssim`` (``utils/ssim.py:29-62``), evaluated in fp64 on the fp32 images.  ``blend``: a float64 plane m; image a is
    replaced by b + m (a - b) first.  ``windows``: ``msssim_windows(H, W, device)`` if the caller kept it.  H, W >= 32."""
    a, b, views = _metric_pair("msssim_terms", a, b)
    c, h, w = a.shape
    if h < 32 or w < 32:
        raise ValueError("msssim_terms: the five levels need an image of at least 32 x 32, not %d x %d" % (h, w))
    m = _plane2(blend, h, w) if blend is not None else None
    if windows is None:
        windows = msssim_windows(h, w, a.device)
    if not (windows.is_cuda and windows.dtype == torch.float64 and tuple(windows.shape) == (MSSSIM_LEVELS, MSSSIM_WINDOW ** 2) and windows.is_contiguous()):
        raise ValueError("msssim_terms: windows must be the float64 device tensor of msssim_windows")
    lib = _sr()
    nbytes = lib.isrMetricsMsssimWorkspace(c, h, w)
    if nbytes <= 0:
        raise RuntimeError("isrMetricsMsssimWorkspace refuses %d x %d x %d" % (c, h, w))
    workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(2 * MSSSIM_LEVELS + 1, dtype=torch.float64, device=a.device)
    rc = lib.isrMetricsMsssim(*views, _ptr(m), m.stride(0) if m is not None else 0, c, h, w, _ptr(windows), _ptr(workspace), _ptr(out), _stream())
    if rc != 0:
        raise RuntimeError("isrMetricsMsssim failed (%d)" % rc)
    return out


def histogram_edges(bins, device):
    """float64 ``np.linspace(0, 1, bins + 1)`` on the device: the edge table of ``abs_diff_histogram``."""
    return torch.from_numpy(np.linspace(0.0, 1.0, bins + 1)).to(device)


def abs_diff_histogram(a, b, bins, scale=1.0, blend=None, edges=None):
    """-> int64 device tensor [bins + 1]: ``np.histogram(scale * sum_c |a_c - b_c|, bins, range=(0, 1))`` in fp64 (channels summed left
    to right) and, last, the number of values inside [0, 1].  ``blend`` as in ``msssim_terms``; ``edges``: ``histogram_edges(bins, device)``
    if the caller kept it."""
    a, b, views = _metric_pair("abs_diff_histogram", a, b)
    c, h, w = a.shape
    if not 1 <= bins <= 1024:
        raise ValueError("abs_diff_histogram: 1 .. 1024 bins")
    m = _plane2(blend, h, w) if blend is not None else None
    if edges is None:
        edges = histogram_edges(bins, a.device)
    if not (edges.is_cuda and edges.dtype == torch.float64 and tuple(edges.shape) == (bins + 1,) and edges.is_contiguous()):
        raise ValueError("abs_diff_histogram: edges must be the float64 device tensor of histogram_edges(bins)")
    counts = torch.empty(bins + 1, dtype=torch.int64, device=a.device)
    rc = _sr().isrMetricsAbsDiffHistogram(*views, _ptr(m), m.stride(0) if m is not None else 0, c, h, w, float(scale), bins, _ptr(edges),
                                          _ptr(counts), _stream())
    if rc != 0:
        raise RuntimeError("isrMetricsAbsDiffHistogram failed (%d)" % rc)
    return counts
