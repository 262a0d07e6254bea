"""Generates tests/golden/colour_reference.npz: the reference's shaded (colour) networks, frame by frame.

The reference's Python modules (`models`, `utils`) are IMPORTED from a checkout of the reference (its SuperresolutionNetwork
directory, given on the command line), unmodified, in the manner of make_sr_fixtures.py (torch CPU, fp32, one thread, deterministic algorithms, `F.grid_sample` forced to `align_corners=True`).
Its `inference` package cannot be imported (cv2 is absent), so `colour_step` below restates `inference/loadedmodel.py:97-119` around
the reference's own `initialImage`, `VideoTools` and `EnhanceNet`; it takes an ALREADY hole-filled flow (the reference fills with
cv.inpaint; this package's `inference.flowfill.fill_flow` is its replacement and is what fills the flows stored here).

No network weights are stored (3.6 MB): the generator and the tests fill the state dict from the same `numpy.random.RandomState`
stream -- `fill_state_dict`, restated in tests/colour_common.py: for every key in `state_dict()` order, a weight [o, i, 3, 3] is
`gain * sqrt(2 / (9 i)) * standard_normal` (He scale; gain 1 except 0.25 for the SECOND convolution of every residual block, which
keeps the ten-block residual stream at the magnitude it starts with) and a bias is `0.05 * standard_normal`.

Content: one 12-channel low-resolution sequence (FRAMES frames, H x W) and its filled flows; for the four input variants
(c = 8, 7, 5, 4 own channels) with initial image "zero", and for c = 8 with "input" as well, per frame: the assembled network input,
the prediction, and `cpu32_vs_fp64_single_step` -- the distance of the reference's fp32 prediction from the same single step evaluated
in fp64 (from the same fp32 previous frame).  The recurrence feeds back clamp(prediction, 0, 1) (mainVideo.py:416).

Run:  python tests/golden/make_colour_fixtures.py <reference checkout>/SuperresolutionNetwork
"""
import argparse
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "colour_reference.npz")
H, W, FRAMES = 8, 12, 4                       # 32 x 48 high-resolution: several 8 x 32 tail tiles, a ragged right column of tiles
WEIGHT_SEED = 20
VARIANTS = ((8, "zero"), (7, "zero"), (5, "zero"), (4, "zero"), (8, "input"))
PREMISE = 4e-5                                # fp32 against fp64, single step: the project's premise for its 1e-4 comparisons


def fill_state_dict(net, seed):
    rs = np.random.RandomState(seed)
    sd = net.state_dict()
    for key, t in sd.items():
        if t.dim() == 4:
            o, i = t.shape[0], t.shape[1]
            gain = 0.25 if (key.startswith("blocks.") and key.endswith(".2.weight")) else 1.0
            v = rs.standard_normal(tuple(t.shape)) * (gain * np.sqrt(2.0 / (9.0 * i)))
        else:
            v = rs.standard_normal(tuple(t.shape)) * 0.05
        sd[key] = torch.from_numpy(v.astype(np.float32))
    net.load_state_dict(sd)
    return net


def make_sequence():
    """A disc that moves over a textured background-free frame: r g b mask nx ny nz depth fx fy ao shadow, as the renderer delivers
    them (mask 0 / 1, normals in [-1, 1], colours slightly outside [0, 1] at highlights so that the c = 8 clamp acts)."""
    rs = np.random.RandomState(7)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    tex = rs.rand(3, H + 8, W + 8)
    frames = []
    for k in range(FRAMES):
        cy, cx = 0.45 * H + 0.3 * k, 0.4 * W + 0.8 * k
        d2 = ((yy - cy) / (0.42 * H)) ** 2 + ((xx - cx) / (0.36 * W)) ** 2
        mask = (d2 < 1.0).astype(np.float64)
        nz = np.sqrt(np.clip(1.0 - d2, 0.0, 1.0))
        nx, ny = (xx - cx) / (0.36 * W), (yy - cy) / (0.42 * H)
        n = np.stack([nx, ny, nz]) * mask
        rgb = (tex[:, k:k + H, 2 * k:2 * k + W] * 0.9 + 0.25 * nz ** 8) * mask          # up to ~1.15 at the highlight
        depth = (0.3 + 0.5 * (1.0 - nz)) * mask
        flow = np.stack([np.full((H, W), 0.8 / W) + 0.01 * nx, np.full((H, W), 0.3 / H) - 0.01 * ny]) * mask
        ao = (0.6 + 0.4 * nz) * mask
        frames.append(np.concatenate([rgb, mask[None], n, depth[None], flow, ao[None], mask[None]], axis=0))
    return torch.from_numpy(np.stack(frames).astype(np.float32))                         # [FRAMES, 12, H, W]


def colour_step(utils, VideoTools, net, low, flow_filled, prev_high, c, mode):
    """inference/loadedmodel.py:97-119 for one frame; returns (network input, prediction)."""
    if c == 8:
        inp = torch.clamp(low[:, 0:8], 0, 1)
    elif c == 7:
        inp = low[:, 0:7]
    elif c == 5:
        inp = torch.cat((low[:, 0:4], low[:, 7:8]), dim=1)
    else:
        inp = low[:, 0:4]
    if prev_high is None:
        prev_high = utils.initialImage(inp, 3, mode, 4)            # (:110, as the reference calls it)
    warped = VideoTools.warp_upscale(prev_high, flow_filled, 4, special_mask=False)
    net_in = torch.cat((inp, VideoTools.flatten_high(warped, 4)), dim=1)
    prediction, _ = net(net_in)
    return net_in, prediction


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    F.grid_sample = functools.partial(F.grid_sample, align_corners=True)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from isosurfacesuperresolution_amd.inference.flowfill import fill_flow       # this package's replacement of cv.inpaint
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "models")):
        sys.exit("usage: make_colour_fixtures.py <reference checkout>/SuperresolutionNetwork")
    sys.path.insert(0, sys.argv[1])
    import models
    import utils
    from models import VideoTools

    opt = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
    low = make_sequence()
    flows = torch.cat([fill_flow(low[k:k + 1, 8:10], low[k:k + 1, 3:4] != 0) for k in range(FRAMES)], dim=0)
    out = {"low": low.numpy(), "flow_filled": flows.numpy(), "weight_seed": np.int64(WEIGHT_SEED),
           "variants": np.array(["%d:%s" % v for v in VARIANTS])}
    worst = 0.0
    with torch.no_grad():
        for c, mode in VARIANTS:
            net = fill_state_dict(models.createNetwork('EnhanceNet', 4, c + 48, [0, 1, 2], 3, opt).eval(), WEIGHT_SEED)
            net64 = fill_state_dict(models.createNetwork('EnhanceNet', 4, c + 48, [0, 1, 2], 3, opt).eval(), WEIGHT_SEED).double()
            tag = "c%d_%s" % (c, mode)
            prev, ins, preds, dist = None, [], [], []
            for k in range(FRAMES):
                net_in, pred = colour_step(utils, VideoTools, net, low[k:k + 1], flows[k:k + 1], prev, c, mode)
                _, pred64 = colour_step(utils, VideoTools, net64, low[k:k + 1].double(), flows[k:k + 1].double(),
                                        None if prev is None else prev.double(), c, mode)
                dist.append((pred.double() - pred64).abs().max().item())
                ins.append(net_in.numpy()[0]); preds.append(pred.numpy()[0])
                prev = torch.clamp(pred, 0, 1)
            out[tag + "_input"] = np.stack(ins)
            out[tag + "_prediction"] = np.stack(preds)
            out[tag + "_cpu32_vs_fp64_single_step"] = np.array(dist)
            out[tag + "_checksums"] = np.array([[a.astype(np.float64).sum(), np.abs(a).astype(np.float64).sum()] for a in preds])
            print(tag, "fp32 vs fp64 single step:", ["%.2e" % d for d in dist],
                  "prediction range [%.3f, %.3f]" % (float(np.min(preds)), float(np.max(preds))))
            worst = max(worst, max(dist))
    assert worst <= PREMISE, "the reference itself is %g from fp64: lower the weight scale" % worst
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; worst fp32-fp64 distance %.2e" % worst)


if __name__ == "__main__":
    main()
