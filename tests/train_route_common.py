"""What the tests of the training graph's convolutions share (test_train_routes_cpu.py, test_train_routes_gpu.py and the autograd-level
tests that state their route): the observation of which kernel family and which kernel form a call took, and the fp64 definitions of
the two operations ``ops._train_conv`` computes.

Routes are decided in two places.  ``ops._train_conv`` picks the FAMILY -- "bf16", "split" or "exact" -- and tallies it in
``ops.FLOP_TALLY``; the library then picks the kernel FORM from the launch's size, and the profiler records its name
(``ops.profile_records``; the low-precision launches are not recorded, for those the tally is the evidence).  Every form of one
layer computes the same numbers, so a comparison of values alone cannot see a case that took another route than it was written for:
each test asserts what ``observed`` returns."""
import os

import torch
import torch.nn.functional as F

ROWS2 = "conv3x3_split_rows2_kernel"
TILE = "conv3x3_split_kernel<false>"
STREAM = "conv3x3_split_stream_kernel"
BLOCK2 = "conv3x3_split_block2_kernel"
ROWSPLIT = "conv3x3_rowsplit_kernel"
TILE4 = "conv3x3_fwd2_kernel<false,1>"
TILE16 = "conv3x3_fwd2_kernel<false,4>"
SPLIT_FORMS = (ROWS2, TILE, STREAM, BLOCK2)
EXACT_FORMS = (ROWSPLIT, TILE4, TILE16, "conv3x3_small_cout_kernel")


def observed(fn):
    """(fn(), {family: algorithmic flops} of ``ops.FLOP_TALLY``, [kernel name] of ``ops.profile_records()``) for the launches ``fn``
    made; the tally and the profiler are back where they were afterwards, whatever ``fn`` did."""
    from isosurfacesuperresolution_amd import ops
    saved_tally, was_profiling = ops.FLOP_TALLY, ops.profile_is_on()
    torch.cuda.synchronize()
    ops.FLOP_TALLY = {}
    ops.profile_enable(True)
    try:
        result = fn()
        torch.cuda.synchronize()
        families = dict(ops.FLOP_TALLY)
        names = [r[0] for r in ops.profile_records()]
    finally:
        ops.profile_enable(was_profiling)
        ops.FLOP_TALLY = saved_tally
    return result, families, names


def fwd64(x, w, b=None, act='none', res=None):
    """act(conv3x3(x, w) + b) + res in fp64; act: 'none' or 'relu'."""
    if act not in ('none', 'relu'):
        raise ValueError(act)
    y = F.conv2d(x.double(), w.double(), b.double() if b is not None else None, padding=1)
    if act == 'relu':
        y = torch.relu(y)
    return y + res.double() if res is not None else y


def dgrad64(g, w, gate=None, skip=None):
    """The gradient of conv3x3(., w) with respect to its input, given the gradient g of its output, in fp64: the convolution of g with
    the weights transposed in their channel pair and flipped in both taps.  ``gate``: the output of a ReLU that produced the input
    (the gradient passes where it is positive); ``skip``: the gradient arriving over a skip connection around the layer."""
    y = F.conv2d(g.double(), w.double().flip(2, 3).transpose(0, 1), padding=1)
    if gate is not None:
        y = torch.where(gate.double() > 0, y, torch.zeros_like(y))
    return y + skip.double() if skip is not None else y


def record_error(case, op, route, kernel, error, normalised, bar):
    """One row of the error table (profiles/train_routes_errors.md) appended to the file ISR_TRAIN_ROUTES_REPORT names, if it names one."""
    path = os.environ.get("ISR_TRAIN_ROUTES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("| %s | %s | %s | %s | %.2e | %.2e | %s |\n" % (case, op, route, kernel if kernel else "(not recorded)", error, normalised, bar))
