"""Shared by tests/test_tecogan_cpu.py and tests/test_tecogan_gpu.py: the reference fixture of the TecoGAN generator
(tests/golden/make_tecogan_fixtures.py -> tests/golden/tecogan_reference.npz) and the weights it was generated with."""
import argparse
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "tecogan_reference.npz"))
SEQ = np.load(os.path.join(GOLDEN, "colour_reference.npz"))          # the sequence the fixture was made from: `low`, `flow_filled`
PREMISE = 4e-5          # fp32 against fp64, single step, of the reference itself: the project's premise for its 1e-4 comparisons
BOUND = 1e-4            # the project's standing single-step tolerance against the reference
CASES = {"a": dict(cin=56, mask=[0, 1, 2], cout=3, recon="residual", blocks=10),
         "b": dict(cin=56, mask=[0, 1, 2], cout=3, recon="residual", blocks=2),
         "c": dict(cin=101, mask=[0, 1, 2, 3, 4], cout=6, recon="direct", blocks=10)}


def fill_state_dict(net, seed):
    """The rule of tests/colour_common.py (the weights are not stored): the same ``numpy.random.RandomState(seed)`` stream as the
    generator -- for every key in ``state_dict()`` order a weight [a, b, 3, 3] is ``gain * sqrt(2 / (9 b)) * standard_normal`` (He
    scale; gain 1, and 0.25 for the second convolution of every residual block), a bias ``0.05 * standard_normal``."""
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


def options(case, upsample='bilinear'):
    c = CASES[case]
    return argparse.Namespace(upsample=upsample, reconType=c["recon"], useBN=False, numResidualLayers=c["blocks"])


def tecogan_net(case, upsample='bilinear'):
    from isosurfacesuperresolution_amd import models
    c = CASES[case]
    net = models.createNetwork('TecoGAN', 4, c["cin"], c["mask"], c["cout"], options(case, upsample)).eval()
    return fill_state_dict(net, int(G["weight_seed"]))
