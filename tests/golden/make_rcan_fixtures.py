"""Generates tests/golden/rcan_reference.npz: the reference's RCAN generator (models/rcan.py), the full 10 x 20 network, frame by frame.

The reference's Python modules (`models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork directory,
given on the command line), unmodified, in the manner of make_tecogan_fixtures.py (torch CPU, fp32, one thread, deterministic
algorithms, `F.grid_sample` forced to `align_corners=True`).  The sequence is the one of colour_reference.npz (`low`, `flow_filled`:
4 frames of 8 x 12), which must exist.

No network weights are stored: the generator and the tests fill the state dict from the same `numpy.random.RandomState` stream --
`fill_state_dict`, restated in tests/rcan_common.py.  For every key in `state_dict()` order, n = standard_normal(shape):
  convolution weight [a, b, 3, 3]   gain * sqrt(2 / (9 b)) * n  (He scale); gain 0.25 for every block's second convolution (`.pre.2.`) and
                                    for the `post` layers of the groups and of `net.rir`, 0.1 for `net.post`, 1 otherwise
  Linear weight [a, b]              6 * n / sqrt(b)  (on this sequence the pooled means are smaller than on a uniform random input: with 3 only
                                    14 % of the gates leave [0.25, 0.75], with 6 about half do; fp32 against fp64 stays near 1e-6)
  `net.post.bias`                   0.5 + 0.05 * n
  every other bias                  0.05 * n
The rule has to meet three conditions on this sequence, asserted below:
  (i)   the reference's fp32 result is within 4e-5 of the same single step in fp64 -- on the output AND on the 64-channel tensor after
        `net.rir` (a small last layer must not mute the 412 layers in front of it);
  (ii)  at least a quarter of all gates lie outside [0.25, 0.75] (a kernel that ignores the attention cannot pass);
  (iii) at most 5 % of the output values are clamped.

Cases, per frame the network input, the prediction (clamped), the unclamped output, the tensor after `net.rir`, and
`cpu32_vs_fp64_single_step` for the output and for the `rir` tensor; of frame 0 every block's gate vector [200, 64]:
  a  colour, c = 8 own channels (56 in, 3 out, mask [0, 1, 2]); recurrent over the 4 frames, feeding back the clamped prediction
     (mainVideo.py:416); initial image "zero";
  b  colour, c = 4 own channels (52 in, 3 out), the first frame only.
Also the `state_dict` keys and shapes of each case's network.

Run:  python tests/golden/make_rcan_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rcan_reference.npz")
SRC = os.path.join(HERE, "colour_reference.npz")
WEIGHT_SEED = 47
PREMISE = 4e-5                                # fp32 against fp64, single step: the project's premise for its 1e-4 comparisons
CASES = {"a": dict(cin=56, own=8, mask=[0, 1, 2], cout=3),
         "b": dict(cin=52, own=4, mask=[0, 1, 2], cout=3)}
LINEAR_GAIN = 6.0


def fill_state_dict(net, seed):
    rs = np.random.RandomState(seed)
    sd = net.state_dict()
    for key, t in sd.items():
        n = rs.standard_normal(tuple(t.shape))
        if t.dim() == 4:
            if key == "net.post.weight":
                gain = 0.1
            elif ".pre.2." in key or key.endswith(".post.weight"):
                gain = 0.25
            else:
                gain = 1.0
            v = n * (gain * np.sqrt(2.0 / (9.0 * t.shape[1])))
        elif t.dim() == 2:
            v = n * (LINEAR_GAIN / np.sqrt(t.shape[1]))
        elif key == "net.post.bias":
            v = 0.5 + 0.05 * n
        else:
            v = 0.05 * n
        sd[key] = torch.from_numpy(v.astype(np.float32))
    net.load_state_dict(sd)
    return net


def make_net(models, case):
    c = CASES[case]
    return fill_state_dict(models.createNetwork('RCAN', 4, c["cin"], c["mask"], c["cout"], None).eval(), WEIGHT_SEED)


def colour_input(utils, VideoTools, low, flow_filled, prev_high, own):
    inp = torch.clamp(low[:, 0:8], 0, 1) if own == 8 else low[:, 0:4]
    if prev_high is None:
        prev_high = utils.initialImage(inp, 3, "zero", False, 4)
    warped = VideoTools.warp_upscale(prev_high, flow_filled, 4, special_mask=False)
    return torch.cat((inp, VideoTools.flatten_high(warped, 4)), dim=1)


def run(net, x):
    """-> (prediction, unclamped output, tensor after net.rir, gates [blocks, 64]) of one forward pass of the reference's network."""
    seen = {"gates": []}
    hooks = [net.net['rir'].register_forward_hook(lambda m, i, o: seen.__setitem__("rir", o.detach().clone()))]
    hooks.append(net.net['post'].register_forward_hook(lambda m, i, o: seen.__setitem__("raw", o.detach().clone())))
    for group in net.net['rir'].blocks:
        for block in group.blocks:
            hooks.append(block.ca.upscaling.register_forward_hook(lambda m, i, o: seen["gates"].append(torch.sigmoid(o.detach())[0])))
    pred, _ = net(x)
    for h in hooks:
        h.remove()
    return pred, seen["raw"], seen["rir"], torch.stack(seen["gates"])


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_rcan_fixtures.py <reference checkout>/SuperresolutionNetwork")
    sys.path.insert(0, sys.argv[1])
    import models
    import utils
    from models import VideoTools

    src = np.load(SRC)
    low, flows = torch.from_numpy(src["low"]), torch.from_numpy(src["flow_filled"])
    out = {"weight_seed": np.int64(WEIGHT_SEED)}
    worst = 0.0
    with torch.no_grad():
        for case, c in CASES.items():
            net, net64 = make_net(models, case), make_net(models, case).double()
            out[case + "_keys"] = np.array(["%s:%s" % (k, ",".join(str(d) for d in t.shape)) for k, t in net.state_dict().items()])
            frames = range(low.shape[0]) if case == "a" else range(1)
            prev, ins, preds, raws, rirs, dist, dist_rir = None, [], [], [], [], [], []
            for k in frames:
                net_in = colour_input(utils, VideoTools, low[k:k + 1], flows[k:k + 1], prev, c["own"])
                pred, raw, rir, gates = run(net, net_in)
                _, raw64, rir64, _ = run(net64, net_in.double())
                dist.append((raw.double() - raw64).abs().max().item())
                dist_rir.append((rir.double() - rir64).abs().max().item())
                ins.append(net_in.numpy()[0]); preds.append(pred.numpy()[0]); raws.append(raw.numpy()[0]); rirs.append(rir.numpy()[0])
                if k == 0:
                    out[case + "_gates_frame0"] = gates.numpy()
                    outside = float(((gates < 0.25) | (gates > 0.75)).float().mean())
                    assert outside >= 0.25, "case %s: only %.1f %% of the gates lie outside [0.25, 0.75]" % (case, 100 * outside)
                clamped = float(((raw < 0) | (raw > 1)).float().mean())
                assert clamped <= 0.05, "case %s frame %d: %.1f %% of the output is clamped" % (case, k, 100 * clamped)
                print(case, k, "fp32 vs fp64: output %.2e, rir %.2e; rir max |v| %.3g; gates outside [0.25, 0.75] %.1f %%; clamped %.2f %%"
                      % (dist[-1], dist_rir[-1], float(rir.abs().max()), 100 * outside, 100 * clamped))
                prev = pred
            out[case + "_input"] = np.stack(ins)
            out[case + "_prediction"] = np.stack(preds)
            out[case + "_output"] = np.stack(raws)
            out[case + "_rir"] = np.stack(rirs)
            out[case + "_cpu32_vs_fp64_single_step"] = np.array(dist)
            out[case + "_rir_cpu32_vs_fp64_single_step"] = np.array(dist_rir)
            worst = max(worst, max(dist), max(dist_rir))
    assert worst <= PREMISE, "the reference itself is %g from fp64: lower the weight scale" % worst
    np.savez_compressed(OUT, **out)
    assert os.path.getsize(OUT) < 1000000, os.path.getsize(OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e" % worst)


if __name__ == "__main__":
    main()
