"""Generates tests/golden/tecogan_reference.npz: the reference's TecoGAN generator (models/tecogan.py), frame by frame.

The reference's Python modules (`models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork
directory, given on the command line), unmodified, in the manner of make_colour_fixtures.py (torch CPU, fp32, one thread,
deterministic algorithms, `F.grid_sample` forced to `align_corners=True`).  The sequence is the one of colour_reference.npz (`low`,
`flow_filled`: 4 frames of 8 x 12), which must exist.

No network weights are stored: the generator and the tests fill the state dict from the same `numpy.random.RandomState` stream --
`fill_state_dict`, restated in tests/tecogan_common.py (the rule of tests/colour_common.py: He scale, gain 0.25 for the second
convolution of every residual block, biases 0.05 * standard_normal; the transposed convolutions' weights [ci, co, 3, 3] take their
fan from dimension 1 like every other weight).

Cases, per frame the network input, the prediction and `cpu32_vs_fp64_single_step` (the distance of the reference's fp32 prediction
from the same single step in fp64):
  a  colour, c = 8 own channels (56 in, 3 out, mask [0, 1, 2]), residual, bilinear, 10 blocks; recurrent over the 4 frames, feeding
     back clamp(prediction, 0, 1) (mainVideo.py:416); initial image "zero";
  b  the same with numResidualLayers = 2, the first frame only;
  c  unshaded 101 -> 6 (mask [0 .. 4]), direct, 10 blocks, the first frame: input = (mask * 2 - 1, normal, depth) + the flattened
     warped initial image "input" (inference/loadedmodel.py:66-96).
Also the `state_dict` keys and shapes of each case's network.

Run:  python tests/golden/make_tecogan_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tecogan_reference.npz")
SRC = os.path.join(HERE, "colour_reference.npz")
WEIGHT_SEED = 31
PREMISE = 4e-5                                # fp32 against fp64, single step: the project's premise for its 1e-4 comparisons
CASES = {"a": dict(cin=56, mask=[0, 1, 2], cout=3, recon="residual", blocks=10),
         "b": dict(cin=56, mask=[0, 1, 2], cout=3, recon="residual", blocks=2),
         "c": dict(cin=101, mask=[0, 1, 2, 3, 4], cout=6, recon="direct", blocks=10)}


def fill_state_dict(net, seed):
    rs = np.random.RandomState(seed)
    sd = net.state_dict()
    for key, t in sd.items():
        if t.dim() == 4:
            gain = 0.25 if (key.startswith("blocks.") and key.endswith(".2.weight")) else 1.0
            v = rs.standard_normal(tuple(t.shape)) * (gain * np.sqrt(2.0 / (9.0 * t.shape[1])))
        else:
            v = rs.standard_normal(tuple(t.shape)) * 0.05
        sd[key] = torch.from_numpy(v.astype(np.float32))
    net.load_state_dict(sd)
    return net


def make_net(models, case):
    c = CASES[case]
    opt = argparse.Namespace(upsample='bilinear', reconType=c["recon"], useBN=False, numResidualLayers=c["blocks"])
    return fill_state_dict(models.createNetwork('TecoGAN', 4, c["cin"], c["mask"], c["cout"], opt).eval(), WEIGHT_SEED)


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


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_tecogan_fixtures.py <reference checkout>/SuperresolutionNetwork")
    sys.path.insert(0, sys.argv[1])
    import models
    import utils
    from models import VideoTools

    src = np.load(SRC)
    low, flows = torch.from_numpy(src["low"]), torch.from_numpy(src["flow_filled"])
    out = {"weight_seed": np.int64(WEIGHT_SEED)}
    worst = 0.0
    with torch.no_grad():
        for case in CASES:
            net, net64 = make_net(models, case), make_net(models, case).double()
            out[case + "_keys"] = np.array(["%s:%s" % (k, ",".join(str(d) for d in t.shape)) for k, t in net.state_dict().items()])
            frames = range(low.shape[0]) if case == "a" else range(1)
            prev, ins, preds, dist = None, [], [], []
            for k in frames:
                if case == "c":
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
            out[case + "_cpu32_vs_fp64_single_step"] = np.array(dist)
            print(case, "fp32 vs fp64 single step:", ["%.2e" % d for d in dist],
                  "prediction range [%.3f, %.3f]" % (float(np.min(preds)), float(np.max(preds))))
            worst = max(worst, max(dist))
    assert worst <= PREMISE, "the reference itself is %g from fp64: lower the weight scale" % worst
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e" % worst)


if __name__ == "__main__":
    main()
