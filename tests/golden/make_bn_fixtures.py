"""Generates tests/golden/bn_reference.npz: the reference's EnhanceNet with `--useBN` (models/enhancenet.py:99-106: ten residual blocks
of conv, BatchNorm2d, ReLU, conv, BatchNorm2d), in eval mode frame by frame and in train mode for one step.

The reference's Python modules (`models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork
directory, given on the command line), unmodified, in the manner of make_tecogan_fixtures.py (torch CPU, fp32, one thread,
deterministic algorithms, `F.grid_sample` forced to `align_corners=True`).  The sequence is the one of colour_reference.npz (`low`,
`flow_filled`: 4 frames of 8 x 12), which must exist.

No network weights are stored: the generator and the tests fill the state dict from the same `numpy.random.RandomState` stream --
`fill_state_dict`, restated in tests/bn_common.py: in `state_dict()` order a convolution weight is He scale * standard_normal (gain
0.25 for `blocks.*.3.weight`, the second convolution of a block), a batch-norm weight 0.5 + U[0, 1), every bias 0.05 *
standard_normal, a running mean 0.3 * standard_normal, a running variance 0.5 + 1.5 * U[0, 1), `num_batches_tracked` 0.  Case t's
batch and cotangent are not stored either (`train_batch`, restated likewise).

Cases:
  a  unshaded 101 -> 6 (mask [0 .. 4]), residual, eval mode: the first frame's input (initial image "input") and prediction;
  b  colour 56 -> 3 (mask [0, 1, 2]), residual, eval mode: four recurrent frames feeding back clamp(prediction, 0, 1);
  t  the network of a in TRAIN mode: one batch [3, 101, 8, 8], loss = sum(prediction * cotangent [3, 6, 32, 32]); the prediction, the
     gradients of blocks.0.0.weight, blocks.0.0.bias, blocks.0.1.{weight,bias}, blocks.9.4.{weight,bias}, postblock.8.weight and of the
     input, and running_mean / running_var of blocks.0.1 and blocks.9.4 after the call.
Every tensor comes with `cpu32_vs_fp64`, the distance of the reference's fp32 result from the same computation in fp64 (the stored
tensors are the fp32 ones, except in case t, where the fp64 results are stored rounded to fp32: the tests of the training step measure
against fp64).  Premises asserted here: predictions <= 4e-5; gradients and statistics <= 4e-5 * max|ref| -- except blocks.0.0.bias, the
bias of a convolution in front of a batch norm, whose gradient is mathematically ZERO (1e-13 in fp64, rounding noise in fp32): it is
held against 1e-4 * max|grad blocks.0.0.weight|, absolutely.

Run:  python tests/golden/make_bn_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "bn_reference.npz")
SRC = os.path.join(HERE, "colour_reference.npz")
WEIGHT_SEED = 47
BATCH_SEED = 48
PREMISE = 4e-5                                # fp32 against fp64: the project's premise for its 1e-4 comparisons
CASES = {"a": dict(cin=101, mask=[0, 1, 2, 3, 4], cout=6),
         "b": dict(cin=56, mask=[0, 1, 2], cout=3)}
CASES["t"] = CASES["a"]
GRAD_KEYS = ("blocks.0.0.weight", "blocks.0.0.bias", "blocks.0.1.weight", "blocks.0.1.bias", "blocks.9.4.weight", "blocks.9.4.bias",
             "postblock.8.weight")
STAT_KEYS = ("blocks.0.1.running_mean", "blocks.0.1.running_var", "blocks.9.4.running_mean", "blocks.9.4.running_var")
ZERO_GRAD = "blocks.0.0.bias"


def fill_state_dict(net, seed):
    rs = np.random.RandomState(seed)
    sd = net.state_dict()
    for key, t in sd.items():
        shape = tuple(t.shape)
        if key.endswith("num_batches_tracked"):
            sd[key] = torch.zeros_like(t)
            continue
        if t.dim() == 4:
            gain = 0.25 if (key.startswith("blocks.") and key.endswith(".3.weight")) else 1.0
            v = rs.standard_normal(shape) * (gain * np.sqrt(2.0 / (9.0 * t.shape[1])))
        elif key.endswith("running_mean"):
            v = rs.standard_normal(shape) * 0.3
        elif key.endswith("running_var"):
            v = 0.5 + 1.5 * rs.random_sample(shape)
        elif key.endswith("weight"):              # a batch-norm weight
            v = 0.5 + rs.random_sample(shape)
        else:
            v = rs.standard_normal(shape) * 0.05
        sd[key] = torch.from_numpy(v.astype(np.float32))
    net.load_state_dict(sd)
    return net


def train_batch():
    """Case t: the batch [3, 101, 8, 8] (0.5 * standard_normal) and the cotangent [3, 6, 32, 32] (standard_normal / 64)."""
    rs = np.random.RandomState(BATCH_SEED)
    x = (rs.standard_normal((3, 101, 8, 8)) * 0.5).astype(np.float32)
    cot = (rs.standard_normal((3, 6, 32, 32)) / 64.0).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(cot)


def make_net(models, case):
    c = CASES[case]
    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=True, numResidualLayers=10)
    return fill_state_dict(models.createNetwork('EnhanceNet', 4, c["cin"], c["mask"], c["cout"], opt).eval(), WEIGHT_SEED)


def colour_input(utils, VideoTools, low, flow_filled, prev_high):
    inp = torch.clamp(low[:, 0:8], 0, 1)
    if prev_high is None:
        prev_high = utils.initialImage(inp, 3, "zero", False, 4)
    warped = VideoTools.warp_upscale(prev_high, flow_filled, 4, special_mask=False)
    return torch.cat((inp, VideoTools.flatten_high(warped, 4)), dim=1)


def unshaded_input(utils, VideoTools, low, flow_filled):
    inp = torch.cat((low[:, 3:4] * 2 - 1, low[:, 4:8]), dim=1)
    prev_high = utils.initialImage(inp, 6, "input", False, 4)
    warped = VideoTools.warp_upscale(prev_high, flow_filled, 4, special_mask=True)
    return torch.cat((inp, VideoTools.flatten_high(warped, 4)), dim=1)


def train_case(net, x, cot):
    """-> {name: tensor} of one train-mode call: prediction, the gradients, the running statistics afterwards."""
    net.train()
    x = x.clone().requires_grad_(True)
    pred, _ = net(x)
    (pred * cot).sum().backward()
    params = dict(net.named_parameters())
    buffers = dict(net.named_buffers())
    res = {"prediction": pred.detach(), "grad_input": x.grad.detach()}
    for k in GRAD_KEYS:
        res["grad_" + k] = params[k].grad.detach()
    for k in STAT_KEYS:
        res[k] = buffers[k].detach().clone()
    return res


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_bn_fixtures.py <reference checkout>/SuperresolutionNetwork")
    sys.path.insert(0, sys.argv[1])
    import models
    import utils
    from models import VideoTools

    src = np.load(SRC)
    low, flows = torch.from_numpy(src["low"]), torch.from_numpy(src["flow_filled"])
    out = {"weight_seed": np.int64(WEIGHT_SEED), "batch_seed": np.int64(BATCH_SEED)}
    with torch.no_grad():
        for case in ("a", "b"):
            net, net64 = make_net(models, case), make_net(models, case).double()
            out[case + "_keys"] = np.array(["%s:%s" % (k, ",".join(str(d) for d in t.shape)) for k, t in net.state_dict().items()])
            frames = range(low.shape[0]) if case == "b" else range(1)
            prev, ins, preds, dist = None, [], [], []
            for k in frames:
                if case == "a":
                    net_in = unshaded_input(utils, VideoTools, low[k:k + 1], flows[k:k + 1])
                else:
                    net_in = colour_input(utils, VideoTools, low[k:k + 1], flows[k:k + 1], prev)
                pred, _ = net(net_in)
                pred64, _ = net64(net_in.double())
                dist.append((pred.double() - pred64).abs().max().item())
                ins.append(net_in.numpy()[0]); preds.append(pred.numpy()[0])
                prev = torch.clamp(pred, 0, 1)
            out[case + "_input"] = np.stack(ins)
            out[case + "_prediction"] = np.stack(preds)
            out[case + "_cpu32_vs_fp64"] = np.array(dist)
            print(case, "fp32 vs fp64 single step:", ["%.2e" % d for d in dist],
                  "prediction range [%.3f, %.3f]" % (float(np.min(preds)), float(np.max(preds))))
            assert max(dist) <= PREMISE, "the reference itself is %g from fp64: lower the weight scale" % max(dist)
    x, cot = train_batch()
    r32 = train_case(make_net(models, "t"), x, cot)
    r64 = train_case(make_net(models, "t").double(), x.double(), cot.double())
    wscale = r64["grad_blocks.0.0.weight"].abs().max().item()
    for name, ref in r64.items():
        err = (r32[name].double() - ref).abs().max().item()
        scale = ref.abs().max().item()
        out["t_" + name] = ref.float().numpy()
        out["t_" + name + "_cpu32_vs_fp64"] = np.float64(err)
        if name == "prediction":
            ok, what = err <= PREMISE, "absolute"
        elif name == "grad_" + ZERO_GRAD:
            ok, what = err <= 1e-4 * wscale and scale <= 1e-4 * wscale, "zero gradient, against 1e-4 max|grad blocks.0.0.weight| = %.2e" % (1e-4 * wscale)
        else:
            ok, what = err <= PREMISE * scale, "relative %.2e" % (err / scale)
        print("t %-32s fp32 vs fp64 %.2e  max|ref| %.3e  (%s)" % (name, err, scale, what))
        assert ok, "the reference's own fp32 %s is %g from fp64 (max|ref| %g)" % (name, err, scale)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
