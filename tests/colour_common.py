"""Shared by tests/test_colour_cpu.py and tests/test_colour_gpu.py: the reference fixture of the colour networks
(tests/golden/make_colour_fixtures.py -> tests/golden/colour_reference.npz) and the weights it was generated with."""
import argparse
import os

import numpy as np
import torch

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colour_reference.npz"))
OPT = argparse.Namespace(upsample='bilinear', reconType='residual', useBN=False, numResidualLayers=10)
VARIANTS = [(int(v.split(":")[0]), v.split(":")[1]) for v in G["variants"]]          # (own channels c, initial image mode)
FRAMES = G["low"].shape[0]
PREMISE = 4e-5          # fp32 against fp64, single step, of the reference itself: the project's premise for its 1e-4 comparisons
BOUND = 1e-4            # the project's standing single-step tolerance against the reference


def fill_state_dict(net, seed):
    """The weights are not stored (3.6 MB): the same ``numpy.random.RandomState(seed)`` stream as the generator -- for every key in
    ``state_dict()`` order a weight [o, i, 3, 3] is ``gain * sqrt(2 / (9 i)) * standard_normal`` (He scale; gain 1, and 0.25 for the
    second convolution of every residual block), a bias ``0.05 * standard_normal``."""
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


def colour_net(c, seed=None):
    from isosurfacesuperresolution_amd import models
    net = models.createNetwork('EnhanceNet', 4, c + 48, [0, 1, 2], 3, OPT).eval()
    return fill_state_dict(net, int(G["weight_seed"]) if seed is None else seed)


def previous_of(tag, k):
    """What the caller feeds back for frame k: the fixture's frame k - 1, clamped (teacher forcing)."""
    return None if k == 0 else torch.from_numpy(G[tag + "_prediction"][k - 1:k]).clamp(0, 1)
